! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_gvn_driver: feeds the *unmodified* getvdep_nests of the reference (getvdep_nests.f90 with getrb.f90, getrc.f90,
! raerod.f90, psih.f90, partdep.f90, caldate.f90, ew.f90; modules par_mod -- the variant with maxnests = 1 -- and com_mod),
! compiled where they lie by tests/golden/make_getvdep_nests_golden.py, with the inputs of a synthetic case on nested grid
! l = 1 and writes the deposition velocities it returns, column by column as the DRYDEP block of calcpar_nests does
! (calcpar_nests.f90:139-155: the roughness length of water from ustarn, the relative humidity from ew, the call, the copy
! into vdepn).  This file is our own code.
!
! Usage:  gvnref_rK in.bin out.bin [reps]
!   in:  nxn, nyn, nspec, wftime (i4); bdate, dy, ylat0, dyn, ylat0n (f8: the MOTHER grid's dy, ylat0 -- the ones
!        getvdep_nests reads -- and the nest's own, which it does not); then f8 arrays in Fortran order:
!        xlandusen(nxn,nyn,numclass), z0(numclass), ri(5,numclass), rac(5,numclass), rcl, rgs, rlu(maxspec,5,numclass), rm,
!        reldiff, henry, f0, density, dryvel(maxspec), vset, schmi, fract(maxspec,ni), and ustarn, olin, psn, tt2n, td2n,
!        ssrn, lsprecn, convprecn, sdn (nxn,nyn)
!   out: vdepn(nxn,nyn,nspec) (f8)
!   reps > 0: the grid is computed reps times and the seconds per pass are printed (the table z0 is restored each pass)
program gvnref
  use par_mod
  use com_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hx, hy, hs, ht
  real(kind=8) :: hb, hdy, hlat, hdyn, hlatn
  real(kind=8), allocatable :: b3(:,:,:), b2(:,:), o(:,:,:)
  real(kind=8) :: bz(numclass), b5(5,numclass), br(maxspec,5,numclass), bs(maxspec), bn(maxspec,ni)
  real :: vd(maxspec), rh, ew, z07
  integer :: ix, jy, i, k, reps, rep, c0, c1, crate
  integer, parameter :: n = 1, l = 1
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  reps = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) reps
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hx, hy, hs, ht
  read(31) hb, hdy, hlat, hdyn, hlatn
  if (hx > nxmaxn .or. hy > nymaxn .or. hs > maxspec .or. maxnests < 1) stop 'gvnref: case larger than par_mod'
  nspec = hs; DRYDEP = .true.; bdate = hb; dy = hdy; ylat0 = hlat; wftime(n) = ht
  numbnests = 1; nxn(l) = hx; nyn(l) = hy; dyn(l) = hdyn; ylat0n(l) = hlatn
  allocate(b3(hx,hy,numclass), b2(hx,hy), o(hx,hy,hs))
  read(31) b3
  xlandusen(:,:,:,l) = 0.
  xlandusen(0:hx-1,0:hy-1,:,l) = b3
  read(31) bz; z0 = bz
  read(31) b5; ri = b5
  read(31) b5; rac = b5
  read(31) br; rcl = br
  read(31) br; rgs = br
  read(31) br; rlu = br
  read(31) bs; rm = bs
  read(31) bs; reldiff = bs
  read(31) bs; henry = bs
  read(31) bs; f0 = bs
  read(31) bs; density = bs
  read(31) bs; dryvel = bs
  read(31) bn; vset = bn
  read(31) bn; schmi = bn
  read(31) bn; fract = bn
  do k = 1, 9
    read(31) b2
    select case (k)
    case (1); ustarn(0:hx-1,0:hy-1,1,n,l) = b2
    case (2); olin(0:hx-1,0:hy-1,1,n,l) = b2
    case (3); psn(0:hx-1,0:hy-1,1,n,l) = b2
    case (4); tt2n(0:hx-1,0:hy-1,1,n,l) = b2
    case (5); td2n(0:hx-1,0:hy-1,1,n,l) = b2
    case (6); ssrn(0:hx-1,0:hy-1,1,n,l) = b2
    case (7); lsprecn(0:hx-1,0:hy-1,1,n,l) = b2
    case (8); convprecn(0:hx-1,0:hy-1,1,n,l) = b2
    case (9); sdn(0:hx-1,0:hy-1,1,n,l) = b2
    end select
  end do
  close(31)
  z07 = z0(7)
  call system_clock(c0, crate)
  do rep = 1, max(reps, 1)
    do jy = 0, nyn(l)-1
      do ix = 0, nxn(l)-1
        ! what getvdep_nests is handed per column: the water roughness from the friction velocity into class 7 of the shared
        ! table, the relative humidity from the two saturation pressures, the Obukhov length, the total rain rate
        z0(7) = 0.016*ustarn(ix,jy,1,n,l)*ustarn(ix,jy,1,n,l)/ga
        rh = ew(td2n(ix,jy,1,n,l))/ew(tt2n(ix,jy,1,n,l))
        call getvdep_nests(n, ix, jy, ustarn(ix,jy,1,n,l), tt2n(ix,jy,1,n,l), psn(ix,jy,1,n,l), 1./olin(ix,jy,1,n,l), &
             ssrn(ix,jy,1,n,l), rh, lsprecn(ix,jy,1,n,l)+convprecn(ix,jy,1,n,l), sdn(ix,jy,1,n,l), vd, l)
        vdepn(ix,jy,1:nspec,n,l) = vd(1:nspec)
      end do
    end do
    z0(7) = z07
  end do
  call system_clock(c1)
  if (reps > 0) print '(a,es12.5)', 'seconds_per_field ', real(c1-c0, kind=8)/real(crate, kind=8)/real(reps, kind=8)
  do i = 1, hs
    o(:,:,i) = vdepn(0:hx-1,0:hy-1,i,n,l)
  end do
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(32) o
  close(32)
end program gvnref
