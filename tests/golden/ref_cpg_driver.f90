! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_cpg_driver: feeds the *unmodified* calcpar (calcpar.f90, with obukhov.f90, richardson.f90, scalev.f90, ew.f90, qvsat.f90
! and calcpv.f90) of the reference -- compiled where they lie by tests/golden/make_cpg_golden.py together with par_mod, com_mod
! and our stand-in for class_gribfile (class_gribfile_standin.f90) -- with the level input and the surface analysis of a
! synthetic case, one record per call, and writes ustar, wstar, oli, hmix and tropopause of the slot after each call.  The
! calls of one run share com_mod, as in the model: tropopause of a slot keeps what the routine does not overwrite.  DRYDEP is
! false, so getvdep is linked (the chain the getvdep pin compiles) but never called.  This file is our own code: it fills
! com_mod, calls the routine and writes arrays.
!
! Usage:  cpgref_rK in.bin out.bin [reps]
!   in:  nx, ny, nz, xglobal, nglobal, sglobal, ncalls, metdata_format, lsubgrid (i4); dx, dy, xlon0, ylat0 (f8);
!        akz, bkz, akm, bkm (f8, nz each); excessoro (f8, nx*ny);
!        then per call: slot (i4), ps, tt2, td2, surfstr, sshf, hmix (f8, nx*ny), tth, qvh, uuh, vvh (f8, nx*ny*nz, x fastest)
!   out: per call: ustar, wstar, oli, hmix, tropopause (f8, nx*ny)
!   reps > 0: every call is made reps times (hmix restored before each) and the seconds per call of the last record are printed
! calcpv keeps automatic arrays of the full par_mod size on the stack: the caller raises the stack limit.
program cpgref
  use par_mod
  use com_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hx, hy, hz, hg(3), hcalls, hfmt, hsub, hslot
  real(kind=8) :: hgeo(4)
  real(kind=8), allocatable :: b1(:), b2(:,:), b3(:,:,:), hm(:,:)
  real, allocatable :: uuh(:,:,:), vvh(:,:,:), pvh(:,:,:)
  integer :: reps, rep, icall, n, metdata_format
  integer(kind=8) :: c0, c1, crate

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  reps = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) reps
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  read(31) hx, hy, hz, hg, hcalls, hfmt, hsub
  read(31) hgeo
  if (hx > nxmax .or. hy > nymax .or. hz > nuvzmax .or. hz > nwzmax) stop 'cpgref: grid larger than par_mod'
  nx = hx; ny = hy; nz = hz; nuvz = hz; nwz = hz; nxfield = hx
  nxmin1 = nx-1; nymin1 = ny-1
  dx = hgeo(1); dy = hgeo(2); xlon0 = hgeo(3); ylat0 = hgeo(4)
  xglobal = (hg(1) /= 0); nglobal = (hg(2) /= 0); sglobal = (hg(3) /= 0)
  metdata_format = hfmt
  lsubgrid = hsub
  DRYDEP = .false.
  numbnests = 0
  allocate(b1(hz), b2(hx,hy), b3(hx,hy,hz), hm(hx,hy))
  akz = 0.; bkz = 0.; akm = 0.; bkm = 0.
  read(31) b1; akz(1:hz) = b1
  read(31) b1; bkz(1:hz) = b1
  read(31) b1; akm(1:hz) = b1
  read(31) b1; bkm(1:hz) = b1
  excessoro = 0.
  read(31) b2; excessoro(0:hx-1,0:hy-1) = b2
  allocate(uuh(0:nxmax-1,0:nymax-1,nuvzmax), vvh(0:nxmax-1,0:nymax-1,nuvzmax), pvh(0:nxmax-1,0:nymax-1,nuvzmax))
  ustar = 0.; wstar = 0.; oli = 0.; hmix = 0.; tropopause = 0.

  do icall = 1, hcalls
    read(31) hslot
    n = hslot
    uuh = 0.; vvh = 0.; pvh = 0.
    ps(:,:,1,n) = 0.; tt2(:,:,1,n) = 0.; td2(:,:,1,n) = 0.; surfstr(:,:,1,n) = 0.; sshf(:,:,1,n) = 0.
    tth(:,:,:,n) = 0.; qvh(:,:,:,n) = 0.
    read(31) b2; ps(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; tt2(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; td2(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; surfstr(0:hx-1,0:hy-1,1,n) = b2
    read(31) b2; sshf(0:hx-1,0:hy-1,1,n) = b2
    read(31) hm
    read(31) b3; tth(0:hx-1,0:hy-1,1:hz,n) = b3
    read(31) b3; qvh(0:hx-1,0:hy-1,1:hz,n) = b3
    read(31) b3; uuh(0:hx-1,0:hy-1,1:hz) = b3
    read(31) b3; vvh(0:hx-1,0:hy-1,1:hz) = b3
    call system_clock(c0, crate)
    do rep = 1, max(reps, 1)
      hmix(0:hx-1,0:hy-1,1,n) = hm
      call calcpar(n, uuh, vvh, pvh, metdata_format)
    end do
    call system_clock(c1)
    call put2(ustar(:,:,1,n)); call put2(wstar(:,:,1,n)); call put2(oli(:,:,1,n)); call put2(hmix(:,:,1,n))
    call put2(tropopause(:,:,1,n))
  end do
  close(31)
  close(32)
  if (reps > 0) print '(a,es12.5)', 'seconds_per_field ', real(c1-c0, kind=8)/real(crate, kind=8)/real(reps, kind=8)

contains
  subroutine put2(a)
    real, intent(in) :: a(0:nxmax-1,0:nymax-1)
    b2 = a(0:hx-1,0:hy-1)
    write(32) b2
  end subroutine put2
end program cpgref
