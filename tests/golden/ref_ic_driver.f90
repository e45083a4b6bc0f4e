! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_ic_driver: feeds the *unmodified* initial_cond_calc and initial_cond_output of the reference (initial_cond_calc.f90,
! initial_cond_output.f90; modules par_mod, com_mod, point_mod, outg_mod, unc_mod), compiled where they lie by
! tests/golden/make_initcond_golden.py, with the prepared particles of flexpart_amd.synthetic.initcond_case() the way the
! end of the run does (timemanager.f90:735-737: the call for every particle, the routine's own itra1 test decides; :745: the
! output), and writes init_cond before the files.  init_cond is allocated and zeroed as outgrid_init.f90:296,329 does.
! This file is our own code.
!
! Usage:  icref_rK in.bin out.bin outdir/
!   in:  i4: nx, ny, nz, n, numxgrid, numygrid, numzgrid, nspec, maxpointspec_act, ioutputforeachrelease, mdomainfill,
!            linit_cond, ind_rel, itime, memind(1), memind(2)
!        f8: dx, dy, xlon0, ylat0, dxout, dyout, outlon0, outlat0, height(nz), outheight(numzgrid),
!            rho(nx,ny,nz) of the physical slots 1 and 2, xmass(maxpointspec_act,nspec), rho_rel(maxpointspec_act),
!            xt(n), yt(n), zt(n), xmass1(n,nspec)
!        i4: npoint(n), itra1(n)
!   out: init_cond(numxgrid,numygrid,numzgrid,nspec,maxpointspec_act) as f8
program icref
  use par_mod
  use com_mod
  use point_mod
  use outg_mod
  use unc_mod
  implicit none
  character(len=512) :: fin, fout, fdir
  integer(kind=4) :: hi(16)
  integer(kind=4), allocatable :: ip(:), ia(:)
  real(kind=8) :: hg(8)
  real(kind=8), allocatable :: b1(:), b3(:,:,:), bx(:), bm(:,:), bq(:,:), o(:)
  integer :: n, itime, j, m
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  call get_command_argument(3, fdir)
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hi
  nx = hi(1); ny = hi(2); nz = hi(3); n = hi(4)
  numxgrid = hi(5); numygrid = hi(6); numzgrid = hi(7); nspec = hi(8); maxpointspec_act = hi(9)
  ioutputforeachrelease = hi(10); mdomainfill = hi(11); linit_cond = hi(12); ind_rel = hi(13); itime = hi(14)
  memind(1) = hi(15); memind(2) = hi(16)
  if (nx > nxmax .or. ny > nymax .or. nz > nzmax .or. n > maxpart .or. nspec > maxspec) stop 'icref: case larger than par_mod'
  nxmin1 = nx-1; nymin1 = ny-1
  read(31) hg
  dx = hg(1); dy = hg(2); xlon0 = hg(3); ylat0 = hg(4); dxout = hg(5); dyout = hg(6); outlon0 = hg(7); outlat0 = hg(8)
  xoutshift = xlon0-outlon0          ! readoutgrid.f90:199-200
  youtshift = ylat0-outlat0
  allocate(b1(nz)); read(31) b1; height = 0.; height(1:nz) = b1
  deallocate(b1); allocate(b1(numzgrid), outheight(numzgrid)); read(31) b1; outheight = b1
  allocate(b3(nx,ny,nz))
  rho = 0.
  do m = 1, 2
    read(31) b3; rho(0:nx-1,0:ny-1,1:nz,m) = b3
  end do
  allocate(bq(maxpointspec_act,nspec), xmass(maxpointspec_act,maxspec), rho_rel(maxpointspec_act))
  read(31) bq; xmass = 0.; xmass(:,1:nspec) = bq
  deallocate(b1); allocate(b1(maxpointspec_act)); read(31) b1; rho_rel = b1
  allocate(xtra1(n), ytra1(n), ztra1(n), xmass1(n,maxspec), npoint(n), itra1(n))
  numpart = n
  allocate(bx(n), bm(n,nspec), ip(n), ia(n))
  read(31) bx; xtra1(1:n) = bx
  read(31) bx; ytra1(1:n) = bx
  read(31) bx; ztra1(1:n) = bx
  read(31) bm; xmass1 = 0.; xmass1(1:n,1:nspec) = bm
  read(31) ip; npoint(1:n) = ip
  read(31) ia; itra1(1:n) = ia
  close(31)
  allocate(init_cond(0:numxgrid-1,0:numygrid-1,numzgrid,maxspec,maxpointspec_act))   ! outgrid_init.f90:296
  init_cond = 0.
  allocate(sparse_dump_r(numxgrid*numygrid*numzgrid), sparse_dump_i(numxgrid*numygrid*numzgrid))
  do j = 1, numpart                                                                  ! timemanager.f90:735-737
    if (linit_cond.ge.1) call initial_cond_calc(itime, j)
  end do
  allocate(o(numxgrid*numygrid*numzgrid*nspec*maxpointspec_act))
  o = reshape(real(init_cond(:,:,:,1:nspec,:), kind=8), (/ size(o) /))
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(32) o
  close(32)
  path(2) = trim(fdir)
  length(2) = len_trim(fdir)
  call initial_cond_output(itime)
end program icref
