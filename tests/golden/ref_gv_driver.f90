! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! ref_gv_driver: feeds the *unmodified* getvdep of the reference (getvdep.f90 with getrb.f90, getrc.f90, raerod.f90,
! psih.f90, partdep.f90, caldate.f90, ew.f90; modules par_mod, com_mod), compiled where they lie by
! tests/golden/make_getvdep_golden.py, with the inputs of a synthetic case and writes the deposition velocities it
! returns, column by column as the DRYDEP block of calcpar does (calcpar.f90:171-189: the roughness length of water from
! ustar, the relative humidity from ew, the call, the copy into vdep).  This file is our own code.
!
! Usage:  gvref_rK in.bin out.bin [reps]
!   in:  nx, ny, nspec, wftime (i4); bdate, dy, ylat0 (f8); then f8 arrays in Fortran order: xlanduse(nx,ny,numclass),
!        z0(numclass), ri(5,numclass), rac(5,numclass), rcl, rgs, rlu(maxspec,5,numclass), rm, reldiff, henry, f0, density,
!        dryvel(maxspec), vset, schmi, fract(maxspec,ni), and ustar, oli, ps, tt2, td2, ssr, lsprec, convprec, sd (nx,ny)
!   out: vdep(nx,ny,nspec) (f8)
!   reps > 0: the grid is computed reps times and the seconds per pass are printed (the table z0 is restored each pass)
program gvref
  use par_mod
  use com_mod
  implicit none
  character(len=512) :: fin, fout, arg
  integer(kind=4) :: hx, hy, hs, ht
  real(kind=8) :: hb, hdy, hlat
  real(kind=8), allocatable :: b3(:,:,:), b2(:,:), o(:,:,:)
  real(kind=8) :: bz(numclass), b5(5,numclass), br(maxspec,5,numclass), bs(maxspec), bn(maxspec,ni)
  real :: vd(maxspec), rh, ew, z07, ufr, t2m, obl, rain
  integer :: ix, jy, i, k, reps, rep, c0, c1, crate
  integer, parameter :: n = 1
  call get_command_argument(1, fin)
  call get_command_argument(2, fout)
  reps = 0
  if (command_argument_count() >= 3) then
    call get_command_argument(3, arg)
    read(arg, *) reps
  end if
  open(31, file=trim(fin), access='stream', form='unformatted', status='old')
  read(31) hx, hy, hs, ht
  read(31) hb, hdy, hlat
  if (hx > nxmax .or. hy > nymax .or. hs > maxspec) stop 'gvref: case larger than par_mod'
  nspec = hs; DRYDEP = .true.; bdate = hb; dy = hdy; ylat0 = hlat; wftime(n) = ht
  allocate(b3(hx,hy,numclass), b2(hx,hy), o(hx,hy,hs))
  read(31) b3
  xlanduse = 0.
  xlanduse(0:hx-1,0:hy-1,:) = b3
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
    case (1); ustar(0:hx-1,0:hy-1,1,n) = b2
    case (2); oli(0:hx-1,0:hy-1,1,n) = b2
    case (3); ps(0:hx-1,0:hy-1,1,n) = b2
    case (4); tt2(0:hx-1,0:hy-1,1,n) = b2
    case (5); td2(0:hx-1,0:hy-1,1,n) = b2
    case (6); ssr(0:hx-1,0:hy-1,1,n) = b2
    case (7); lsprec(0:hx-1,0:hy-1,1,n) = b2
    case (8); convprec(0:hx-1,0:hy-1,1,n) = b2
    case (9); sd(0:hx-1,0:hy-1,1,n) = b2
    end select
  end do
  close(31)
  z07 = z0(7)
  call system_clock(c0, crate)
  do rep = 1, max(reps, 1)
    do jy = 0, hy-1
      do ix = 0, hx-1
        ! what getvdep is handed per column: the water roughness from the friction velocity into class 7 of the shared
        ! table, the relative humidity from the two saturation pressures, the Obukhov length, the total rain rate
        ufr = ustar(ix,jy,1,n); t2m = tt2(ix,jy,1,n)
        z0(7) = 0.016*ufr*ufr/ga
        rh = ew(td2(ix,jy,1,n))/ew(t2m)
        obl = 1./oli(ix,jy,1,n)
        rain = lsprec(ix,jy,1,n)+convprec(ix,jy,1,n)
        call getvdep(n, ix, jy, ufr, t2m, ps(ix,jy,1,n), obl, ssr(ix,jy,1,n), rh, rain, sd(ix,jy,1,n), vd)
        vdep(ix,jy,1:nspec,n) = vd(1:nspec)
      end do
    end do
    z0(7) = z07
  end do
  call system_clock(c1)
  if (reps > 0) print '(a,es12.5)', 'seconds_per_field ', real(c1-c0, kind=8)/real(crate, kind=8)/real(reps, kind=8)
  do i = 1, hs
    o(:,:,i) = vdep(0:hx-1,0:hy-1,i,n)
  end do
  open(32, file=trim(fout), access='stream', form='unformatted', status='replace')
  write(32) o
  close(32)
end program gvref
