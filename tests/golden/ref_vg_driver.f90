! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_vg_driver: feeds the *unmodified* verttransform_gfs (verttransform_gfs.f90) of the reference -- compiled where it
! lies by tests/golden/make_vtgfs_golden.py together with par_mod, com_mod, cmapf_mod, ew and qvsat -- with the
! pressure-level input of a synthetic case, one record per call, and writes the z-level arrays com_mod holds after each
! call.  The calls of one run share com_mod, as in the model: height and nmixz come from the first call and ww of a slot
! keeps what the routine does not overwrite.  This file is our own code: it fills com_mod, calls the routine and writes arrays.
!
! Usage:  vgref_rK in.bin out.bin [reps]
!   in:  nx, ny, nz, xglobal, nglobal, sglobal, ncalls (i4); dx, dy, xlon0, ylat0 (f8); akz, bkz, aknew, bknew (f8, nz each);
!        then per call: slot (i4), ps, tt2, td2 (f8, nx*ny), tth, qvh, uuh, vvh, pvh, wwh (f8, nx*ny*nz, x fastest)
!   out: per call: height (f8, nz), nmixz (i4), uu, vv, ww, tt, qv, pv, rho, drhodz, pplev, uupol, vvpol (f8, nx*ny*nz)
!   reps > 0: every call is made reps times and the seconds per call of the last record are printed
! The routine keeps uvwzlev, an automatic array of the full par_mod size, on the stack: the caller raises the stack limit.
program vgref
  use par_mod
  use com_mod
  use cmapf_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hx, hy, hz, hg(3), hcalls, hslot
  real(kind=8) :: hgeo(4)
  real(kind=8), allocatable :: b1(:), b2(:,:), b3(:,:,:)
  real, allocatable :: uuh(:,:,:), vvh(:,:,:), pvh(:,:,:), wwh(:,:,:)
  integer :: reps, rep, icall, n
  integer(kind=8) :: c0, c1, crate
  real :: sizenorth, sizesouth

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  reps = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) reps
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  read(31) hx, hy, hz, hg, hcalls
  read(31) hgeo
  if (hx > nxmax .or. hy > nymax .or. hz > nzmax) stop 'vgref: grid larger than par_mod'
  nx = hx; ny = hy; nz = hz; nuvz = hz; nwz = hz; nxfield = hx
  nxmin1 = nx-1; nymin1 = ny-1
  dx = hgeo(1); dy = hgeo(2); xlon0 = hgeo(3); ylat0 = hgeo(4)
  dxconst = 180./(dx*r_earth*pi)          ! as gridcheck_gfs.f90:241-242
  dyconst = 180./(dy*r_earth*pi)
  xglobal = (hg(1) /= 0); nglobal = (hg(2) /= 0); sglobal = (hg(3) /= 0)
  switchnorthg = 999999.; switchsouthg = 999999.
  ! the polar stereographic maps, call sequence of gridcheck_gfs.f90
  if (sglobal) then
    sizesouth = 6.*(switchsouth+90.)/dy
    call stlmbr(southpolemap, -90., 0.)
    call stcm2p(southpolemap, 0., 0., switchsouth, 0., sizesouth, sizesouth, switchsouth, 180.)
    switchsouthg = (switchsouth-ylat0)/dy
  end if
  if (nglobal) then
    sizenorth = 6.*(90.-switchnorth)/dy
    call stlmbr(northpolemap, 90., 0.)
    call stcm2p(northpolemap, 0., 0., switchnorth, 0., sizenorth, sizenorth, switchnorth, 180.)
    switchnorthg = (switchnorth-ylat0)/dy
  end if
  readclouds = .false.; sumclouds = .false.; numbnests = 0
  lsprec = 0.; convprec = 0.
  allocate(b1(hz), b2(hx,hy), b3(hx,hy,hz))
  read(31) b1; akz(1:hz) = b1
  read(31) b1; bkz(1:hz) = b1
  read(31) b1; aknew(1:hz) = b1
  read(31) b1; bknew(1:hz) = b1
  allocate(uuh(0:nxmax-1,0:nymax-1,nuvzmax), vvh(0:nxmax-1,0:nymax-1,nuvzmax))
  allocate(pvh(0:nxmax-1,0:nymax-1,nuvzmax), wwh(0:nxmax-1,0:nymax-1,nwzmax))
  uu = 0.; vv = 0.; ww = 0.; tt = 0.; qv = 0.; pv = 0.; rho = 0.; drhodz = 0.; pplev = 0.; uupol = 0.; vvpol = 0.

  do icall = 1, hcalls
    read(31) hslot
    n = hslot
    uuh = 0.; vvh = 0.; pvh = 0.; wwh = 0.
    ps(:,:,1,n) = 0.; tt2(:,:,1,n) = 0.; td2(:,:,1,n) = 0.; tth(:,:,:,n) = 0.; qvh(:,:,:,n) = 0.
    read(31) b2; ps(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; tt2(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; td2(0:hx-1,0:hy-1,1,n) = b2
    read(31) b3; tth(0:hx-1,0:hy-1,1:hz,n) = b3
    read(31) b3; qvh(0:hx-1,0:hy-1,1:hz,n) = b3
    read(31) b3; uuh(0:hx-1,0:hy-1,1:hz) = b3
    read(31) b3; vvh(0:hx-1,0:hy-1,1:hz) = b3
    read(31) b3; pvh(0:hx-1,0:hy-1,1:hz) = b3
    read(31) b3; wwh(0:hx-1,0:hy-1,1:hz) = b3
    call system_clock(c0, crate)
    do rep = 1, max(reps, 1)
      call verttransform_gfs(n, uuh, vvh, wwh, pvh)
    end do
    call system_clock(c1)
    b1 = height(1:hz)
    write(32) b1
    write(32) int(nmixz, kind=4)
    call put3(uu(:,:,:,n)); call put3(vv(:,:,:,n)); call put3(ww(:,:,:,n)); call put3(tt(:,:,:,n)); call put3(qv(:,:,:,n))
    call put3(pv(:,:,:,n)); call put3(rho(:,:,:,n)); call put3(drhodz(:,:,:,n)); call put3(pplev(:,:,:,n))
    call put3(uupol(:,:,:,n)); call put3(vvpol(:,:,:,n))
  end do
  close(31)
  close(32)
  if (reps > 0) print '(a,es12.5)', 'seconds_per_field ', real(c1-c0, kind=8)/real(crate, kind=8)/real(reps, kind=8)

contains
  subroutine put3(a)
    real, intent(in) :: a(0:nxmax-1,0:nymax-1,nzmax)
    b3 = a(0:hx-1,0:hy-1,1:hz)
    write(32) b3
  end subroutine put3
end program vgref
