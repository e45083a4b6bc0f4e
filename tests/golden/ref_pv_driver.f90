! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_pv_driver: feeds the *unmodified* calcpv (calcpv.f90) or, built with -DFLEXREF_NESTS against the reference's
! par_mod_meteoswiss.f90 (maxnests = 1), calcpv_nests (calcpv_nests.f90) of the reference -- compiled where they lie by
! tests/golden/make_calcpv_golden.py together with par_mod and com_mod -- with the model-level input of a synthetic case
! and writes the potential vorticity it returns.  This file is our own code.
!
! Usage:  pvref_rK in.bin out.bin [reps]
!   in:  nx, ny, nuvz, xglobal, nglobal, sglobal (i4); dx, dy, ylat0 (f8); then f8 arrays in Fortran order: akz(nuvz),
!        bkz(nuvz), ps(nx,ny), tth(nx,ny,nuvz), uuh(nx,ny,nuvz), vvh(nx,ny,nuvz)
!        (the nest build reads the same record as nxn(1), nyn(1), dxn(1), dyn(1), ylat0n(1), psn, tthn, uuhn, vvhn)
!   out: pvh(nx,ny,nuvz) (f8)
!   reps > 0: the routine is called reps times and the seconds per call are printed
! Both routines keep two automatic arrays of the full par_mod size on the stack: the caller raises the stack limit.
program pvref
  use par_mod
  use com_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hx, hy, hz, hg(3)
  real(kind=8) :: hdx, hdy, hlat
  real(kind=8), allocatable :: b1(:), b2(:,:), b3(:,:,:), o(:,:,:)
#ifdef FLEXREF_NESTS
  real, allocatable :: uuhn(:,:,:,:), vvhn(:,:,:,:), pvhn(:,:,:,:)
#else
  real, allocatable :: uuh(:,:,:), vvh(:,:,:), pvh(:,:,:)
#endif
  integer :: reps, rep, k
  integer(kind=8) :: c0, c1, crate
  integer, parameter :: n = 1
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  reps = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) reps
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hx, hy, hz, hg
  read(31) hdx, hdy, hlat
  if (hz > nuvzmax) stop 'pvref: more levels than par_mod'
  nuvz = hz
  allocate(b1(hz), b2(hx,hy), b3(hx,hy,hz), o(hx,hy,hz))
  read(31) b1; akz(1:hz) = b1
  read(31) b1; bkz(1:hz) = b1
  read(31) b2
#ifdef FLEXREF_NESTS
  if (hx > nxmaxn .or. hy > nymaxn) stop 'pvref: nest larger than par_mod'
  numbnests = 1; nxn(1) = hx; nyn(1) = hy
  dxn(1) = hdx; dyn(1) = hdy; ylat0n(1) = hlat
  call com_mod_allocate_nests
  allocate(uuhn(0:nxmaxn-1,0:nymaxn-1,nuvzmax,maxnests), vvhn(0:nxmaxn-1,0:nymaxn-1,nuvzmax,maxnests))
  allocate(pvhn(0:nxmaxn-1,0:nymaxn-1,nuvzmax,maxnests))
  psn = 0.; tthn = 0.; uuhn = 0.; vvhn = 0.; pvhn = 0.
  psn(0:hx-1,0:hy-1,1,n,1) = b2
  read(31) b3; tthn(0:hx-1,0:hy-1,1:hz,n,1) = b3
  read(31) b3; uuhn(0:hx-1,0:hy-1,1:hz,1) = b3
  read(31) b3; vvhn(0:hx-1,0:hy-1,1:hz,1) = b3
#else
  if (hx > nxmax .or. hy > nymax) stop 'pvref: grid larger than par_mod'
  nx = hx; ny = hy; nxmin1 = nx-1; nymin1 = ny-1
  dx = hdx; dy = hdy; ylat0 = hlat
  xglobal = (hg(1) /= 0); nglobal = (hg(2) /= 0); sglobal = (hg(3) /= 0)
  allocate(uuh(0:nxmax-1,0:nymax-1,nuvzmax), vvh(0:nxmax-1,0:nymax-1,nuvzmax), pvh(0:nxmax-1,0:nymax-1,nuvzmax))
  ps = 0.; tth = 0.; uuh = 0.; vvh = 0.; pvh = 0.
  ps(0:hx-1,0:hy-1,1,n) = b2
  read(31) b3; tth(0:hx-1,0:hy-1,1:hz,n) = b3
  read(31) b3; uuh(0:hx-1,0:hy-1,1:hz) = b3
  read(31) b3; vvh(0:hx-1,0:hy-1,1:hz) = b3
#endif
  close(31)
  call system_clock(c0, crate)
  do rep = 1, max(reps, 1)
#ifdef FLEXREF_NESTS
    call calcpv_nests(1, n, uuhn, vvhn, pvhn)
#else
    call calcpv(n, uuh, vvh, pvh)
#endif
  end do
  call system_clock(c1)
  if (reps > 0) print '(a,es12.5)', 'seconds_per_field ', real(c1-c0, kind=8)/real(crate, kind=8)/real(reps, kind=8)
  do k = 1, hz
#ifdef FLEXREF_NESTS
    o(:,:,k) = pvhn(0:hx-1,0:hy-1,k,1)
#else
    o(:,:,k) = pvh(0:hx-1,0:hy-1,k)
#endif
  end do
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(32) o
  close(32)
end program pvref
