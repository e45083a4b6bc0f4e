! TEST INFRASTRUCTURE ONLY -- never linked into or called by the product path.
!
! A stand-in of our own for the reference's module class_gribfile (gributils/class_gribfile_mod.f90), whose source needs
! ecCodes and therefore does not compile in an image without that library.  calcpar.f90, obukhov.f90 and richardson.f90
! `use class_gribfile` but take nothing from it except the three integer constants that name the centre of the
! meteorological data (class_gribfile_mod.f90:45-47).  With a module of that name that holds those three parameters the
! unmodified routines compile, and tests/golden/make_cpg_golden.py can pin the NCEP and the ECMWF branch of calcpar to them.
! The values are those of the reference; nothing else of its module is restated here.
module class_gribfile
  implicit none
  integer, parameter :: GRIBFILE_CENTRE_NCEP = 1
  integer, parameter :: GRIBFILE_CENTRE_ECMWF = 2
  integer, parameter :: GRIBFILE_CENTRE_UNKNOWN = -9999
end module class_gribfile
