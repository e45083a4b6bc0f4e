! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_oh_driver: feeds the *unmodified* gethourlyOH and ohreaction of the reference (gethourlyOH.f90, ohreaction.f90,
! zenithangle.f90, photo_O1D.f90, caldate.f90; modules par_mod in its maxnests = 1 variant, com_mod, oh_mod), compiled where they lie by
! tests/golden/make_ohreaction_golden.py, with flexpart_amd.synthetic.oh_case() in the order the time manager calls them
! (timemanager.f90:171-172, 212-216), and dumps OH_hourly and memOHtime after every gethourlyOH, xmass1 after every
! ohreaction.  oh_mod is allocated as readOHfield.f90:59-64 does; memOHtime starts at zero, as a static module variable does.
! The nest's geometry is derived as gridcheck_nests.f90:359-372 does.  This file is our own code.
!
! Usage:  ohref_rK in.bin out.bin [ntime]
!   in:  i4: nx, ny, nz, n, nxOH, nyOH, nzOH, nspec, ldirect, ncalls, nxn, nyn
!        f8: dx, dy, xlon0, ylat0, bdate, dxn, dyn, xlon0n, ylat0n, height(nz), lonOH, latOH, altOH, lonjr(360), latjr(180),
!            jrate_average(360,180,12), OH_field(nxOH,nyOH,nzOH,12), tt(nx,ny,nz) of the physical slots 1 and 2,
!            ohcconst, ohdconst, ohnconst (nspec each), xt(n), yt(n), zt(n), xmass1(n,nspec)
!        per call i4: kind (0 gethourlyOH, 1 ohreaction), itime, ltsample, memtime(2), memind(2)
!   out: per gethourlyOH f8 memOHtime(2), OH_hourly(nxOH,nyOH,nzOH,2); per ohreaction f8 xmass1(n,nspec)
!   ntime: after the sequence, one more ohreaction over ntime storage spaces (the case's particles repeated) is timed with
!          cpu_time and the seconds are printed; nothing of it is written.
program ohref
  use par_mod
  use com_mod
  use oh_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hi(12), hc(7)
  real(kind=8) :: hg(9), t0, t1
  real(kind=8), allocatable :: b1(:), b3(:,:,:), b4(:,:,:,:), bj(:,:,:), bx(:), bm(:,:)
  integer :: n, ncalls, ic, itime, ltsample, ntime, j, k
  real :: xaux2, yaux2
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  ntime = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) ntime
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hi
  nx = hi(1); ny = hi(2); nz = hi(3); n = hi(4); nxOH = hi(5); nyOH = hi(6); nzOH = hi(7); nspec = hi(8); ldirect = hi(9)
  ncalls = hi(10); numbnests = 1; nxn(1) = hi(11); nyn(1) = hi(12)
  if (nx > nxmax .or. ny > nymax .or. nz > nzmax .or. nspec > maxspec) stop 'ohref: case larger than par_mod'
  read(31) hg
  dx = hg(1); dy = hg(2); xlon0 = hg(3); ylat0 = hg(4); bdate = hg(5)
  dxn(1) = hg(6); dyn(1) = hg(7); xlon0n(1) = hg(8); ylat0n(1) = hg(9)
  xresoln(0) = 1.; yresoln(0) = 1.                       ! gridcheck_nests.f90:359-372
  xresoln(1) = dx/dxn(1); yresoln(1) = dy/dyn(1)
  xaux2 = xlon0n(1)+real(nxn(1)-1)*dxn(1); yaux2 = ylat0n(1)+real(nyn(1)-1)*dyn(1)
  xln(1) = (xlon0n(1)-xlon0)/dx; xrn(1) = (xaux2-xlon0)/dx
  yln(1) = (ylat0n(1)-ylat0)/dy; yrn(1) = (yaux2-ylat0)/dy
  allocate(b1(nz)); read(31) b1; height = 0.; height(1:nz) = b1; deallocate(b1)
  allocate(lonOH(nxOH), latOH(nyOH), altOH(nzOH), OH_field(nxOH,nyOH,nzOH,12), OH_hourly(nxOH,nyOH,nzOH,2))   ! readOHfield.f90:59-64
  allocate(b1(nxOH)); read(31) b1; lonOH = b1; deallocate(b1)
  allocate(b1(nyOH)); read(31) b1; latOH = b1; deallocate(b1)
  allocate(b1(nzOH)); read(31) b1; altOH = b1; deallocate(b1)
  allocate(b1(360)); read(31) b1; lonjr = b1; deallocate(b1)
  allocate(b1(180)); read(31) b1; latjr = b1; deallocate(b1)
  allocate(bj(360,180,12)); read(31) bj; jrate_average = bj; deallocate(bj)
  allocate(b4(nxOH,nyOH,nzOH,12)); read(31) b4; OH_field = b4; deallocate(b4)
  OH_hourly = 0.; memOHtime = 0.
  allocate(b3(nx,ny,nz))                                 ! (tt is static and zero outside what is set here)
  read(31) b3; tt(0:nx-1,0:ny-1,1:nz,1) = b3
  read(31) b3; tt(0:nx-1,0:ny-1,1:nz,2) = b3
  allocate(b1(nspec))
  ohcconst = 0.; ohdconst = 0.; ohnconst = 0.
  read(31) b1; ohcconst(1:nspec) = b1
  read(31) b1; ohdconst(1:nspec) = b1
  read(31) b1; ohnconst(1:nspec) = b1
  allocate(xtra1(max(n,ntime)), ytra1(max(n,ntime)), ztra1(max(n,ntime)), xmass1(max(n,ntime),maxspec))
  numpart = n
  allocate(bx(n), bm(n,nspec))
  read(31) bx; xtra1(1:n) = bx
  read(31) bx; ytra1(1:n) = bx
  read(31) bx; ztra1(1:n) = bx
  read(31) bm; xmass1 = 0.; xmass1(1:n,1:nspec) = bm
  loutstep = 10800*ldirect
  itime = 0; ltsample = 0
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  do ic = 1, ncalls
    read(31) hc
    itime = hc(2); ltsample = hc(3); memtime(1) = hc(4); memtime(2) = hc(5); memind(1) = hc(6); memind(2) = hc(7)
    if (hc(1) == 0) then
      call gethourlyOH(itime)
      write(32) real(memOHtime, kind=8), real(OH_hourly, kind=8)
    else
      call ohreaction(itime, ltsample, 0)
      write(32) real(xmass1(1:n,1:nspec), kind=8)
    end if
  end do
  close(31)
  close(32)
  if (ntime > 0) then
    do j = n+1, ntime
      k = mod(j-1, n)+1
      xtra1(j) = xtra1(k); ytra1(j) = ytra1(k); ztra1(j) = ztra1(k); xmass1(j,:) = xmass1(k,:)
    end do
    numpart = ntime
    call cpu_time(t0)
    call ohreaction(itime, ltsample, 0)
    call cpu_time(t1)
    write(*,'(a,i0,a,f10.4,a)') 'ohreaction over ', ntime, ' storage spaces: ', t1-t0, ' s on one core'
  end if
end program ohref
