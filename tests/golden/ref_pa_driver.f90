! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_pa_driver: feeds the *unmodified* partpos_average and partoutput_average of the reference (partpos_average.f90,
! partoutput_average.f90, caldate.f90; modules par_mod, com_mod), compiled where they lie by
! tests/golden/make_partavg_golden.py, with the prepared particles of flexpart_amd.synthetic.partavg_case() the way the
! particle loop does (timemanager.f90:537: the particles with itra1 = itime; :617: the call after the move) and then the
! way the output block does (:455).  Before every output call it dumps npart_av and the fourteen sums.  The reference never
! initialises the sums; the driver zeroes them once, as the engine does at creation.  This file is our own code.
!
! Usage:  paref_rK in.bin out.bin outdir/
!   in:  i4: nx, ny, nz, n, nintervals, memtime(2), memind(2), ncalls(nintervals), itime_out(nintervals)
!        f8: dx, dy, xlon0, ylat0, bdate, height(nz), oro(nx,ny),
!            per physical slot 1, 2: pv, qv, tt, uu, vv, rho (nx,ny,nz), tropopause, hmix (nx,ny)
!        per interval: per call: i4 itime; f8 xt(n), yt(n), zt(n); i4 due(n);   then i4 itra1(n) of the output
!   out: per interval: i4 npart_av(n); f8 cartx, carty, cartz, z, topo, pv, qv, tt, uu, vv, rho, tro, hmix, energy (n each)
program paref
  use par_mod
  use com_mod
  implicit none
  character(len=512) :: fin, fout, fdir
  integer(kind=4) :: hi(5), hm(4), it
  integer(kind=4), allocatable :: nc(:), to(:), due(:), ia(:)
  real(kind=8) :: hg(5)
  real(kind=8), allocatable :: b1(:), b2(:,:), b3(:,:,:), bx(:), by(:), bz(:)
  integer :: n, nint, iv, k, j, m, itime
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  call get_command_argument(3, fdir)
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hi
  nx = hi(1); ny = hi(2); nz = hi(3); n = hi(4); nint = hi(5)
  if (nx > nxmax .or. ny > nymax .or. nz > nzmax .or. n > maxpart) stop 'paref: case larger than par_mod'
  nxmin1 = nx-1; nymin1 = ny-1
  read(31) hm
  memtime(1) = hm(1); memtime(2) = hm(2); memind(1) = hm(3); memind(2) = hm(4)
  allocate(nc(nint), to(nint))
  read(31) nc
  read(31) to
  read(31) hg
  dx = hg(1); dy = hg(2); xlon0 = hg(3); ylat0 = hg(4); bdate = hg(5)
  allocate(b1(nz), b2(nx,ny), b3(nx,ny,nz))
  read(31) b1; height = 0.; height(1:nz) = b1
  oro = 0.; pv = 0.; qv = 0.; tt = 0.; uu = 0.; vv = 0.; rho = 0.; tropopause = 0.; hmix = 0.
  read(31) b2; oro(0:nx-1,0:ny-1) = b2
  do m = 1, 2
    read(31) b3; pv(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b3; qv(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b3; tt(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b3; uu(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b3; vv(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b3; rho(0:nx-1,0:ny-1,1:nz,m) = b3
    read(31) b2; tropopause(0:nx-1,0:ny-1,1,m) = b2
    read(31) b2; hmix(0:nx-1,0:ny-1,1,m) = b2
  end do
  ipout = 3
  call com_mod_allocate_part(n)
  numpart = n
  npart_av = 0
  part_av_cartx = 0.; part_av_carty = 0.; part_av_cartz = 0.; part_av_z = 0.; part_av_topo = 0.; part_av_pv = 0.
  part_av_qv = 0.; part_av_tt = 0.; part_av_uu = 0.; part_av_vv = 0.; part_av_rho = 0.; part_av_tro = 0.
  part_av_hmix = 0.; part_av_energy = 0.
  path(2) = trim(fdir)
  length(2) = len_trim(fdir)
  allocate(bx(n), by(n), bz(n), due(n), ia(n))
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  do iv = 1, nint
    do k = 1, nc(iv)
      read(31) it
      itime = it
      read(31) bx
      read(31) by
      read(31) bz
      read(31) due
      do j = 1, n
        if (due(j) /= 0) then
          xtra1(j) = bx(j); ytra1(j) = by(j); ztra1(j) = bz(j)
          call partpos_average(itime, j)
        end if
      end do
    end do
    read(31) ia
    itra1 = ia
    write(32) int(npart_av, kind=4)
    write(32) real(part_av_cartx, kind=8), real(part_av_carty, kind=8), real(part_av_cartz, kind=8), real(part_av_z, kind=8), &
              real(part_av_topo, kind=8), real(part_av_pv, kind=8), real(part_av_qv, kind=8), real(part_av_tt, kind=8), &
              real(part_av_uu, kind=8), real(part_av_vv, kind=8), real(part_av_rho, kind=8), real(part_av_tro, kind=8), &
              real(part_av_hmix, kind=8), real(part_av_energy, kind=8)
    itime = to(iv)
    call partoutput_average(itime)
  end do
  close(31)
  close(32)
end program paref
