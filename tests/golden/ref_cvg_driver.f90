! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_cvg_driver: calls the *unmodified* convmix (convmix.f90) of the reference with metdata_format = GRIBFILE_CENTRE_NCEP --
! and through it the unmodified calcmatrix, CONVECT / TLIFT (convect43c.f90), redist, sort2, f_qvsat, ew, ran3 -- compiled
! where they lie by tests/golden/make_cvg_golden.py together with par_mod, com_mod, conv_mod, flux_mod, outg_mod, random_mod
! and our stand-in for class_gribfile (class_gribfile_standin.f90), on a synthetic case (synthetic.convection_case_gfs).
! This file is our own code: it fills com_mod / conv_mod, calls the routine and writes arrays.
!
! Usage:  cvgref_rK in.bin out.bin
!   in:  nx, ny, nz, nconvlev, ldirect, lsynctime, memtime(1), memtime(2), n, ncalls (i4); height(nz) (f8);
!        ps, tt2, td2 (f8, nx*ny*2), tt, qv, pplev (f8, nx*ny*nz*2, x fastest, slot slowest), cbaseflux (f8, nx*ny),
!        xtra1, ytra1, ztra1 (f8, n), itimes (i4, ncalls), due (i4, n*ncalls)
!   out: mode A, end to end: after each of the ncalls consecutive calls of convmix: ztra1 (f8, n), cbaseflux (f8, nx*ny);
!        mode B, per column, from the start state: the number of columns that hold due particles (i4), then for each of them,
!        after a call of convmix on the particles of that column alone: column = jy*nx+ix, lconv, nconvtop, exit (i4), psconv,
!        the column's new cbaseflux (f8), pconv(1:nuvz), phconv(1:nuvz), dpr, tconv, qconv (1:nuvz-1),
!        fmassfrac(1:nconvlev+1,1:nconvlev+1) (f8).  cbaseflux and ztra1 are restored after each column.
!   lconv is read off fmassfrac: calcmatrix zeroes it and only a convective column fills it (this driver zeroes the whole
!   array before each call, so nothing of another column is left in it).
!   exit: which way CONVECT left before its mixing part, found by calling the reference's CONVECT again on the sounding
!   calcmatrix left in conv_mod -- once with the column's old mass flux, once with a mass flux of 1 (the exit on the buoyancy
!   at cloud base needs a mass flux of zero): 0 none, 1 tconv(nk) < 250 / qconv(nk) <= 0 / ihmin = nl-1 (iflag 0 whatever the
!   mass flux), 2 the lifting condensation level (iflag 2), 3 cloud base at nl-1 or above (iflag 3), 4 not buoyant at cloud
!   base with no mass flux from before (iflag 0 only with a zero mass flux), 5 none of these and yet not convective (old and
!   new mass flux zero).
!   pconv(nuvz) -- read by calcmatrix for phconv(nuvz), written by no GFS run -- is printed as this build holds it.
program cvgref
  use par_mod
  use com_mod
  use conv_mod
  use class_gribfile
  implicit none
  character(len=512) :: fin, fout
  integer(kind=4) :: hdr(10)
  integer :: nxl, nyl, nzl, ncalls, n, ic, i, j, k, itime, nl1, ncolb, ix, jy
  real(kind=8) :: hnz
  real(kind=8), allocatable :: ps8(:,:,:), tt28(:,:,:), td28(:,:,:), tt8(:,:,:,:), qv8(:,:,:,:), pp8(:,:,:,:), cb8(:,:), x8(:), y8(:), z8(:)
  real(kind=8), allocatable :: v8(:), fm8(:,:)
  integer(kind=4), allocatable :: itimes(:), due(:,:), pcol(:)
  logical, allocatable :: visited(:)
  real, allocatable :: zstart(:), cb0(:,:)
  integer(kind=4) :: rec(4)
  integer :: iflag1, iflag2, lc, xcode
  real :: cbold, cbnew, cbp, precip, wd, tprime, qprime, delt, pmin, pmax

  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hdr
  nxl = hdr(1); nyl = hdr(2); nzl = hdr(3); nconvlev = hdr(4); ldirect = hdr(5); lsynctime = hdr(6)
  n = hdr(9); ncalls = hdr(10)
  if (nxl > nxmax .or. nyl > nymax .or. nzl > nzmax .or. nzl > nuvzmax .or. nconvlev > nconvlevmax - 1 .or. n > maxpart) stop 'cvgref: case larger than par_mod'
  read(31) hnz
  allocate(ps8(nxl,nyl,2), tt28(nxl,nyl,2), td28(nxl,nyl,2), tt8(nxl,nyl,nzl,2), qv8(nxl,nyl,nzl,2), pp8(nxl,nyl,nzl,2))
  allocate(cb8(nxl,nyl), x8(n), y8(n), z8(n), itimes(ncalls), due(n,ncalls), pcol(n), visited(0:nxl*nyl-1), zstart(n))
  read(31) ps8, tt28, td28, tt8, qv8, pp8, cb8, x8, y8, z8, itimes, due
  close(31)
  nx = nxl; ny = nyl; nz = nzl; nuvz = nzl; nwz = nzl
  nxmin1 = nx - 1; nymin1 = ny - 1
  numbnests = 0
  iflux = 0
  memtime(1) = hdr(7); memtime(2) = hdr(8); memind(1) = 1; memind(2) = 2
  height(nz) = real(hnz)
  do k = 1, 2
    ps(0:nxl-1,0:nyl-1,1,k) = real(ps8(:,:,k)); tt2(0:nxl-1,0:nyl-1,1,k) = real(tt28(:,:,k)); td2(0:nxl-1,0:nyl-1,1,k) = real(td28(:,:,k))
    tt(0:nxl-1,0:nyl-1,1:nzl,k) = real(tt8(:,:,:,k)); qv(0:nxl-1,0:nyl-1,1:nzl,k) = real(qv8(:,:,:,k))
    pplev(0:nxl-1,0:nyl-1,1:nzl,k) = real(pp8(:,:,:,k))
  end do
  numpart = n
  call com_mod_allocate_part(n)
  do i = 1, n
    xtra1(i) = x8(i); ytra1(i) = y8(i); ztra1(i) = real(z8(i)); zstart(i) = real(z8(i))
  end do
  itramem(1:n) = 0
  cbaseflux = 0.
  allocate(cb0(nxl,nyl))
  cb0 = real(cb8)
  cbaseflux(0:nxl-1,0:nyl-1) = cb0
  print '(a,es24.16)', 'pconv(nuvz) as this build holds it before the first call: ', real(pconv(nuvz), kind=8)

  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  ! ---- mode A: consecutive calls, one lsynctime apart
  do ic = 1, ncalls
    itime = itimes(ic)
    do i = 1, n
      itra1(i) = merge(itime, itime + 12345, due(i, ic) /= 0)
    end do
    call convmix(itime, GRIBFILE_CENTRE_NCEP)
    do i = 1, n
      z8(i) = ztra1(i)
    end do
    cb8 = cbaseflux(0:nxl-1,0:nyl-1)
    write(32) z8, cb8
  end do
  pmin = pconv(nuvz); pmax = pconv(nuvz)

  ! ---- mode B: column by column, from the start state
  itime = itimes(1)
  delt = real(abs(lsynctime))
  nl1 = nconvlev + 1
  allocate(v8(nuvz), fm8(nl1,nl1))
  visited = .false.
  do i = 1, n
    pcol(i) = -1
    if (due(i, 1) /= 0) then
      pcol(i) = nint(real(ytra1(i))) * nxl + nint(real(xtra1(i)))
      visited(pcol(i)) = .true.
    end if
    ztra1(i) = zstart(i)
  end do
  ncolb = count(visited)
  write(32) int(ncolb, kind=4)
  do j = 0, nxl*nyl - 1
    if (.not. visited(j)) cycle
    jy = j / nxl
    ix = j - jy * nxl
    cbaseflux(0:nxl-1,0:nyl-1) = cb0
    cbold = cbaseflux(ix,jy)
    fmassfrac = 0.
    do i = 1, n
      itra1(i) = merge(itime, itime + 12345, pcol(i) == j)
    end do
    call convmix(itime, GRIBFILE_CENTRE_NCEP)
    pmin = min(pmin, pconv(nuvz)); pmax = max(pmax, pconv(nuvz))
    cbnew = cbaseflux(ix,jy)
    lc = 0
    if (any(fmassfrac(1:nl1,1:nl1) /= 0.)) lc = 1
    do k = 1, nl1
      do i = 1, nl1
        fm8(i,k) = fmassfrac(i,k)
      end do
    end do
    rec(1) = j; rec(2) = lc; rec(3) = merge(nconvtop, 0, lc == 1)
    ! the probe calls of CONVECT (conv_mod's sounding is what calcmatrix left); everything recorded was taken before them
    cbp = cbold
    call convect(nconvlevmax, nconvlev, delt, iflag1, precip, wd, tprime, qprime, cbp)
    cbp = 1.
    call convect(nconvlevmax, nconvlev, delt, iflag2, precip, wd, tprime, qprime, cbp)
    xcode = 0
    if (iflag1 == 2) then
      xcode = 2
    else if (iflag1 == 3) then
      xcode = 3
    else if (iflag1 == 0 .and. iflag2 == 0) then
      xcode = 1
    else if (iflag1 == 0) then
      xcode = 4
    else if (lc == 0) then
      xcode = 5
    end if
    rec(4) = xcode
    write(32) rec
    write(32) real(psconv, kind=8), real(cbnew, kind=8)
    v8(1:nuvz) = pconv(1:nuvz); write(32) v8(1:nuvz)
    v8(1:nuvz) = phconv(1:nuvz); write(32) v8(1:nuvz)
    v8(1:nuvz-1) = dpr(1:nuvz-1); write(32) v8(1:nuvz-1)
    v8(1:nuvz-1) = tconv(1:nuvz-1); write(32) v8(1:nuvz-1)
    v8(1:nuvz-1) = qconv(1:nuvz-1); write(32) v8(1:nuvz-1)
    write(32) fm8
    do i = 1, n
      ztra1(i) = zstart(i)
    end do
  end do
  close(32)
  print '(a,2es24.16)', 'pconv(nuvz) over all calls, min and max: ', real(pmin, kind=8), real(pmax, kind=8)

end program cvgref
