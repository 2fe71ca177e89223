"""Model terms beyond WENO advection, mirroring the reference's constructors:

  Centered(order=2)                               src/Advection/centered_reconstruction.jl:39-60 (the reference's default advection)
  FPlane(f=...) / FPlane(rotation_rate, latitude) src/Coriolis/f_plane.jl:8-42
  ScalarDiffusivity([VerticallyImplicitTimeDiscretization()], ν=..., κ=...)
                                                  src/TurbulenceClosures/turbulence_closure_implementations/scalar_diffusivity.jl
  ConvectiveAdjustmentVerticalDiffusivity([time_discretization], convective_κz=..., background_κz=..., convective_νz=..., background_νz=...)
                                                  .../turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl
  RiBasedVerticalDiffusivity([time_discretization], Ri_dependent_tapering=..., horizontal_Ri_filter=..., nu_0=..., kappa_0=..., kappa_ca=..., ...)
                                                  .../turbulence_closure_implementations/ri_based_vertical_diffusivity.jl
  CATKEVerticalDiffusivity([time_discretization], mixing_length=CATKEMixingLength(...), turbulent_kinetic_energy_equation=CATKEEquation(...), ...)
                                                  .../turbulence_closure_implementations/TKEBasedVerticalDiffusivities/
  TKEDissipationVerticalDiffusivity([time_discretization], tke_dissipation_equations=TKEDissipationEquations(...),
                                    stability_functions=VariableStabilityFunctions(...) | ConstantStabilityFunctions(...),
                                    minimum_length_scale=StratifiedDisplacementScale(...), ...)
                                                  .../TKEBasedVerticalDiffusivities/tke_dissipation_*.jl
  Smagorinsky(coefficient=..., Pr=...), SmagorinskyLilly(C=..., Cb=..., Pr=...), LillyCoefficient(...)
                                                  .../turbulence_closure_implementations/Smagorinskys/{smagorinsky,lilly_coefficient}.jl
  BuoyancyTracer(), SeawaterBuoyancy(...), LinearEquationOfState(...)
                                                  src/BuoyancyFormulations/{buoyancy_tracer,seawater_buoyancy,linear_equation_of_state}.jl
  FluxBoundaryCondition, ValueBoundaryCondition, GradientBoundaryCondition, FieldBoundaryConditions, BetaPlane
                                                  src/BoundaryConditions/{boundary_condition,field_boundary_conditions}.jl

Only what the HIP kernels implement is accepted; everything else raises NotImplementedError.
"""
import math

import numpy as np

from . import _lib
from .architectures import on_architecture


def sind(x):
    """Julia's sind (base/special/trig.jl): the argument is reduced mod 360 exactly and the result is the correctly rounded
    sin(x π / 180) -- exactly 0, ±0.5, ±1 where they occur, which math.sin(math.radians(x)) misses (sind(30) == 0.5).
    Used by FPlane(latitude = φ), f = 2 Ω sind(φ) (f_plane.jl:38-40; test/test_coriolis.jl:24-27 expects f = 2 from Ω = 2, φ = 30)."""
    from decimal import Decimal, localcontext
    from fractions import Fraction
    r = Fraction(x) % 360
    sign = 1.0
    if r >= 180:
        r, sign = r - 180, -1.0
    if r > 90:
        r = 180 - r
    if r == 0:
        return 0.0
    if r == 30:
        return sign * 0.5
    if r == 90:
        return sign
    with localcontext() as ctx:
        ctx.prec = 60
        pi = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")
        t = Decimal(r.numerator) / Decimal(r.denominator) * pi / 180
        term, total, n = t, t, 1
        while abs(term) > Decimal(10) ** -58:
            term = -term * t * t / ((2 * n) * (2 * n + 1))
            total += term
            n += 1
        return sign * float(total)


def cosd(x):
    """Julia's cosd: cos(x π / 180) correctly rounded, exact at the multiples of 30 / 90 where the cosine is 0, ±0.5, ±1
    (cosd(x) = sind(90 - x) holds exactly for the reduced argument)."""
    from fractions import Fraction
    return sind(Fraction(90) - Fraction(x))


class Centered:
    """Centered(order=2)"""

    def __init__(self, order=2, grid=None):
        if order % 2 != 0:
            raise ValueError("Centered reconstruction scheme is defined only for even orders")
        if order != 2 or grid is not None:
            raise NotImplementedError("the MI355X backend implements Centered(order=2) only")
        self.order = order
        self.buffer = 1  # required_halo_size

    code = _lib.ADVECTION_CENTERED2

    def __repr__(self):
        return "Centered(order=2)"


class FPlane:
    """FPlane(; f, rotation_rate=Ω_Earth, latitude) (f_plane.jl:23-42)"""
    OMEGA_EARTH = 7.292115e-5  # src/Coriolis/Coriolis.jl

    def __init__(self, f=None, rotation_rate=None, latitude=None):
        if f is not None and latitude is not None:
            raise ValueError("Either both keywords rotation_rate and latitude must be specified, or only f must be specified.")
        if f is None and latitude is None:
            raise ValueError("Either both keywords rotation_rate and latitude must be specified, or only f must be specified.")
        if f is None:
            rotation_rate = self.OMEGA_EARTH if rotation_rate is None else rotation_rate
            f = 2 * rotation_rate * sind(latitude)
        self.f = float(f)


class BetaPlane:
    """BetaPlane(; f₀, β) or BetaPlane(; rotation_rate=Ω_Earth, latitude, radius=R_Earth) (beta_plane.jl:6-41): f = f₀ + β y, evaluated at
    the y node of each velocity point (:43-57)."""
    OMEGA_EARTH = 7.292115e-5  # src/Coriolis/Coriolis.jl:19
    R_EARTH = 6371.0e3         # src/Grids/Grids.jl:40

    def __init__(self, f0=None, beta=None, rotation_rate=None, latitude=None, radius=None, **kw):
        f0 = kw.pop("f₀", f0)
        beta = kw.pop("β", beta)
        if kw:
            raise TypeError(f"unknown keyword(s) {sorted(kw)}")
        use_f_and_beta = f0 is not None and beta is not None
        use_planet = latitude is not None
        if use_f_and_beta == use_planet:
            raise ValueError("Either both keywords f₀ and β must be specified, *or* all of rotation_rate, latitude, and radius.")
        if use_planet:
            rotation_rate = self.OMEGA_EARTH if rotation_rate is None else rotation_rate
            radius = self.R_EARTH if radius is None else radius
            f0 = 2 * rotation_rate * sind(latitude)
            beta = 2 * rotation_rate * cosd(latitude) / radius
        self.f0, self.beta = float(f0), float(beta)


class ExplicitTimeDiscretization:
    """ExplicitTimeDiscretization() (TurbulenceClosures.jl): the closure's fluxes enter the tendencies"""

    def __repr__(self):
        return "ExplicitTimeDiscretization()"


class VerticallyImplicitTimeDiscretization:
    """VerticallyImplicitTimeDiscretization(): the vertical diffusion of u, v, w and the tracers is stepped with backward Euler -- a
    tridiagonal solve per column after every rk3_substep! / ab2_step! (vertically_implicit_diffusion_solver.jl) -- and only the boundary
    fluxes and the horizontal fluxes stay in the tendencies (abstract_scalar_diffusivity_closure.jl:214-260)."""

    def __repr__(self):
        return "VerticallyImplicitTimeDiscretization()"


def as_time_discretization(td):
    """an instance, or one of the strings "Explicit" / "VerticallyImplicit" -> an instance"""
    if isinstance(td, (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)):
        return td
    if td in (ExplicitTimeDiscretization, "Explicit", "ExplicitTimeDiscretization"):
        return ExplicitTimeDiscretization()
    if td in (VerticallyImplicitTimeDiscretization, "VerticallyImplicit", "VerticallyImplicitTimeDiscretization"):
        return VerticallyImplicitTimeDiscretization()
    raise ValueError(f"time_discretization must be ExplicitTimeDiscretization() or VerticallyImplicitTimeDiscretization(), got {td!r}")


def is_vertically_implicit(closure):
    """is_vertically_implicit(closure) (vertically_implicit_diffusion_solver.jl)"""
    return isinstance(getattr(closure, "time_discretization", None), VerticallyImplicitTimeDiscretization)


def implicit_diffusion_solver(closure, grid):
    """implicit_diffusion_solver(time_discretization, grid) (vertically_implicit_diffusion_solver.jl:193-205) reduced to its check: the
    solver itself is a kernel that keeps no state (ocn_implicit_vertical_diffusion_step)."""
    if is_vertically_implicit(closure) and grid.topology[2] != "Bounded":
        raise ValueError("VerticallyImplicitTimeDiscretization can only be specified on grids that are Bounded in the z-direction.")


class ScalarDiffusivity:
    """ScalarDiffusivity([time_discretization]; ν=0, κ=0): ExplicitTimeDiscretization() (default) or
    VerticallyImplicitTimeDiscretization() -- as the first positional argument, as in the reference, or `time_discretization=` (an instance
    or "Explicit" / "VerticallyImplicit") --, ThreeDimensionalFormulation, constant coefficients.
    κ is a number (every tracer) or a dict {tracer name: κ}."""

    def __init__(self, *args, **kw):
        if args and (isinstance(args[0], (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization))
                     or args[0] in (ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)):
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"], args = args[0], args[1:]
        names = ("nu", "kappa", "time_discretization", "formulation")
        if len(args) > len(names):
            raise TypeError(f"ScalarDiffusivity takes at most {len(names)} positional arguments after the time discretization")
        for name, value in zip(names, args):
            if name in kw:
                raise TypeError(f"{name} given twice")
            kw[name] = value
        nu = kw.pop("ν", kw.pop("nu", 0.0))
        kappa = kw.pop("κ", kw.pop("kappa", 0.0))
        time_discretization = kw.pop("time_discretization", "Explicit")
        formulation = kw.pop("formulation", "ThreeDimensional")
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
        self.time_discretization = as_time_discretization(time_discretization)
        if formulation != "ThreeDimensional":
            raise NotImplementedError("only the ThreeDimensionalFormulation (isotropic) is implemented")
        if callable(nu) or callable(kappa) or np.ndim(nu) > 0:  # (numpy scalars are numbers)
            raise NotImplementedError("only constant ν, κ are implemented")
        self.nu = float(nu)
        self.kappa = kappa

    def kappa_of(self, name):
        if isinstance(self.kappa, dict):
            if name not in self.kappa:
                raise ValueError(f"no diffusivity κ given for tracer {name}")
            return float(self.kappa[name])
        return float(self.kappa)


class ConvectiveAdjustmentVerticalDiffusivity:
    """ConvectiveAdjustmentVerticalDiffusivity([time_discretization = VerticallyImplicitTimeDiscretization()];
    convective_κz = 0, convective_νz = 0, background_κz = 0, background_νz = 0)
    (convective_adjustment_vertical_diffusivity.jl:62-70): a VerticalFormulation closure whose tracer diffusivity κᶜ and viscosity κᵘ, fields
    at (Center, Center, Face), take the convective value where ∂z b < 0 and the background value where ∂z b >= 0.  The time discretization
    is the first positional argument or `time_discretization=` (an instance or "Explicit" / "VerticallyImplicit").  ASCII aliases:
    convective_kappa_z, convective_nu_z, background_kappa_z, background_nu_z.  The coefficients are numbers (the reference's kernel puts
    them straight into an ifelse); HydrostaticFreeSurfaceModel only."""
    _NAMES = {"convective_κz": "convective_kappa_z", "convective_νz": "convective_nu_z", "background_κz": "background_kappa_z",
              "background_νz": "background_nu_z"}

    def __init__(self, *args, **kw):
        if len(args) > 1:
            raise TypeError("ConvectiveAdjustmentVerticalDiffusivity takes one positional argument, the time discretization")
        if args:
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"] = args[0]
        self.time_discretization = as_time_discretization(kw.pop("time_discretization", VerticallyImplicitTimeDiscretization()))
        self._given = {}  # the numbers as they were given: the reference's summary prints convective_κz=1 for an integer
        for greek, ascii_name in self._NAMES.items():
            if greek in kw and ascii_name in kw:
                raise TypeError(f"{greek} given twice")
            value = kw.pop(greek, kw.pop(ascii_name, 0.0))
            if isinstance(value, (bool, str)) or callable(value) or not np.isscalar(value) or not np.isreal(value):
                raise NotImplementedError(f"ConvectiveAdjustmentVerticalDiffusivity: {greek} must be a number (functions, arrays, fields and "
                                          "per-tracer tuples are not implemented)")
            setattr(self, ascii_name, float(value))
            self._given[ascii_name] = value
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")

    convective_κz = property(lambda self: self.convective_kappa_z)
    convective_νz = property(lambda self: self.convective_nu_z)
    background_κz = property(lambda self: self.background_kappa_z)
    background_νz = property(lambda self: self.background_nu_z)

    def c_struct(self):
        """struct ocn_convective_adjustment"""
        return _lib.CConvectiveAdjustment(self.convective_kappa_z, self.convective_nu_z, self.background_kappa_z, self.background_nu_z)

    def __repr__(self):  # Base.summary (convective_adjustment_vertical_diffusivity.jl:129-133)
        v = self._given
        return (f"ConvectiveAdjustmentVerticalDiffusivity{{{type(self.time_discretization).__name__}}}(background_κz={v['background_kappa_z']} "
                f"convective_κz={v['convective_kappa_z']} background_νz={v['background_nu_z']} convective_νz={v['convective_nu_z']})")


class PiecewiseLinearRiDependentTapering:
    """1 - min(1, max(0, (Ri - Ri₀) / Riᵟ)) (ri_based_vertical_diffusivity.jl:45, 239)"""
    code = _lib.RI_TAPER_LINEAR

    def __repr__(self):
        return type(self).__name__


class ExponentialRiDependentTapering(PiecewiseLinearRiDependentTapering):
    """exp(-max(0, (Ri - Ri₀) / Riᵟ)) (:46, 240)"""
    code = _lib.RI_TAPER_EXP


class HyperbolicTangentRiDependentTapering(PiecewiseLinearRiDependentTapering):
    """(1 - tanh((Ri - Ri₀) / Riᵟ)) / 2 (:47, 241)"""
    code = _lib.RI_TAPER_TANH


class FivePointHorizontalFilter:
    """filter_horizontally(::FivePointHorizontalFilter) = ℑxyᶜᶜᵃ(ℑxyᶠᶠᵃ Ri) (:54-56)"""

    def __repr__(self):
        return "FivePointHorizontalFilter"


def _prettysummary(x, compact=True):
    """prettysummary(::AbstractFloat) (Grids/grid_utils.jl:278): Julia's shortest representation, compact (at most six significant digits);
    compact = False: string(::Float64), every digit of the shortest representation"""
    from decimal import Decimal
    x = float(x)
    if x != x:
        return "NaN"
    if math.isinf(x):
        return "Inf" if x > 0 else "-Inf"
    if x == 0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    d = Decimal(repr(x))
    if compact and len(d.as_tuple().digits) > 6:
        d = Decimal(f"{x:.5e}")
    sign, digits, exp = d.normalize().as_tuple()
    digits = "".join(map(str, digits))
    point = len(digits) + exp  # the value is 0.digits x 10^point
    if -4 < point <= 6:
        if point <= 0:
            body = "0." + "0" * (-point) + digits
        elif point >= len(digits):
            body = digits + "0" * (point - len(digits)) + ".0"
        else:
            body = digits[:point] + "." + digits[point:]
    else:
        body = digits[0] + "." + (digits[1:] or "0") + "e" + str(point - 1)
    return ("-" if sign else "") + body


class RiBasedVerticalDiffusivity:
    """RiBasedVerticalDiffusivity([time_discretization = VerticallyImplicitTimeDiscretization()]; Ri_dependent_tapering =
    HyperbolicTangentRiDependentTapering(), horizontal_Ri_filter = nothing, minimum_entrainment_buoyancy_gradient = 1e-10,
    maximum_diffusivity = Inf, maximum_viscosity = Inf, ν₀ = 0.7, κ₀ = 0.5, κᶜᵃ = 1.7, Cᵉⁿ = 0.1, Cᵃᵛ = 0.6, Ri₀ = 0.1, Riᵟ = 0.4, warning = true)
    (ri_based_vertical_diffusivity.jl:125-162): a VerticalFormulation closure whose κᶜ and κᵘ, fields at (Center, Center, Face), are
    convective-adjustment, entrainment and shear-mixing coefficients, the last tapered by the Richardson number, averaged in time.

    The canonical keyword names are ASCII: nu_0, kappa_0, kappa_ca, C_en, C_av, Ri_0, Ri_delta.  Keyword names are NFKC-normalised before
    lookup (Python does the same to identifiers in source), so κᶜᵃ=, Cᵉⁿ=, Cᵃᵛ=, Riᵟ= work as written and ν₀, κ₀, Ri₀, which Python does not
    accept in source, through **{"ν₀": ...}.  The parameters are numbers; HydrostaticFreeSurfaceModel only."""
    DEFAULTS = {"nu_0": 0.7, "kappa_0": 0.5, "kappa_ca": 1.7, "C_en": 0.1, "C_av": 0.6, "Ri_0": 0.1, "Ri_delta": 0.4,
                "minimum_entrainment_buoyancy_gradient": 1e-10, "maximum_diffusivity": math.inf, "maximum_viscosity": math.inf}
    # NFKC("ν₀") = "ν0", NFKC("κᶜᵃ") = "κca", NFKC("Riᵟ") = "Riδ", ...
    _NAMES = {"ν0": "nu_0", "κ0": "kappa_0", "κca": "kappa_ca", "Cen": "C_en", "Cav": "C_av", "Ri0": "Ri_0", "Riδ": "Ri_delta"}
    _SHOWN = {"nu_0": "ν₀", "kappa_0": "κ₀", "kappa_ca": "κᶜᵃ", "C_en": "Cᵉⁿ", "C_av": "Cᵃᵛ", "Ri_0": "Ri₀", "Ri_delta": "Riᵟ"}
    WARNING = ("RiBasedVerticalDiffusivity is an experimental turbulence closure that \nis unvalidated and whose default parameters are not "
               "calibrated for \nrealistic ocean conditions or for use in a three-dimensional \nsimulation. Use with caution and report bugs "
               "and problems with physics \nto https://github.com/CliMA/Oceananigans.jl/issues.")

    @classmethod
    def canonical(cls, name):
        """the ASCII name of a keyword or attribute in any spelling, or None"""
        import unicodedata
        n = unicodedata.normalize("NFKC", name)
        return n if n in cls.DEFAULTS else cls._NAMES.get(n)

    def __init__(self, *args, **kw):
        import warnings
        if len(args) > 1:
            raise TypeError("RiBasedVerticalDiffusivity takes one positional argument, the time discretization")
        if args:
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"] = args[0]
        self.time_discretization = as_time_discretization(kw.pop("time_discretization", VerticallyImplicitTimeDiscretization()))
        tapering = kw.pop("Ri_dependent_tapering", None)
        tapering = HyperbolicTangentRiDependentTapering() if tapering is None else (tapering() if isinstance(tapering, type) else tapering)
        if not isinstance(tapering, PiecewiseLinearRiDependentTapering):
            raise TypeError("Ri_dependent_tapering must be PiecewiseLinearRiDependentTapering(), ExponentialRiDependentTapering() or "
                            "HyperbolicTangentRiDependentTapering()")
        self.Ri_dependent_tapering = tapering
        ri_filter = kw.pop("horizontal_Ri_filter", None)
        ri_filter = ri_filter() if isinstance(ri_filter, type) else ri_filter
        if ri_filter is not None and not isinstance(ri_filter, FivePointHorizontalFilter):
            raise TypeError("horizontal_Ri_filter must be None or FivePointHorizontalFilter()")
        self.horizontal_Ri_filter = ri_filter
        warning = kw.pop("warning", True)
        values = dict(self.DEFAULTS)
        seen = set()
        for name, value in kw.items():
            key = self.canonical(name)
            if key is None:
                raise TypeError(f"unexpected keyword arguments {[name]}")
            if key in seen:
                raise TypeError(f"{key} given twice")
            seen.add(key)
            if isinstance(value, (bool, str)) or callable(value) or not np.isscalar(value) or not np.isreal(value):
                raise NotImplementedError(f"RiBasedVerticalDiffusivity: {self._SHOWN.get(key, key)} must be a number (functions, arrays, fields "
                                          "and per-tracer tuples are not implemented)")
            values[key] = float(value)
        for key, value in values.items():
            setattr(self, key, value)
        if warning:
            warnings.warn(self.WARNING, stacklevel=2)

    def __getattr__(self, name):  # the reference's field names in any spelling: closure.κᶜᵃ, getattr(closure, "ν₀")
        key = type(self).canonical(name) if not name.startswith("_") else None
        if key is None or key == name:
            raise AttributeError(name)
        return getattr(self, key)

    def c_struct(self):
        """struct ocn_ri_based"""
        return _lib.CRiBased(self.nu_0, self.kappa_0, self.kappa_ca, self.C_en, self.C_av, self.Ri_0, self.Ri_delta,
                             self.minimum_entrainment_buoyancy_gradient, self.maximum_diffusivity, self.maximum_viscosity,
                             self.Ri_dependent_tapering.code,
                             _lib.RI_FILTER_NONE if self.horizontal_Ri_filter is None else _lib.RI_FILTER_FIVE_POINT)

    def __repr__(self):  # Base.show (ri_based_vertical_diffusivity.jl:347-361)
        rows = [("Ri_dependent_tapering", repr(self.Ri_dependent_tapering))]
        rows += [(self._SHOWN[k], _prettysummary(getattr(self, k))) for k in ("kappa_0", "nu_0", "kappa_ca", "C_en", "C_av", "Ri_0", "Ri_delta")]
        rows += [(k, _prettysummary(getattr(self, k))) for k in ("maximum_diffusivity", "maximum_viscosity")]
        lines = [f"RiBasedVerticalDiffusivity{{{type(self.time_discretization).__name__}}}"]
        lines += [("└── " if n == len(rows) - 1 else "├── ") + f"{name}: {value}" for n, (name, value) in enumerate(rows)]
        return "\n".join(lines)


class _Coefficients:
    """a Base.@kwdef struct of numbers: ASCII keyword names are canonical, the reference's spellings are accepted after NFKC normalisation
    (which Python applies to identifiers in source: Cʰⁱu= arrives as Chiu) and through **{...} where Python takes no such identifier"""
    DEFAULTS, SPELLINGS = {}, {}

    @classmethod
    def canonical(cls, name):
        import unicodedata
        if name in cls.DEFAULTS:
            return name
        n = unicodedata.normalize("NFKC", name)
        for ascii_name, spelling in cls.SPELLINGS.items():
            if n == unicodedata.normalize("NFKC", spelling):
                return ascii_name
        return None

    def __init__(self, **kw):
        values, seen = dict(self.DEFAULTS), set()
        for name, value in kw.items():
            key = self.canonical(name)
            if key is None:
                raise TypeError(f"{type(self).__name__}: unexpected keyword arguments {[name]}")
            if key in seen:
                raise TypeError(f"{type(self).__name__}: {key} given twice")
            seen.add(key)
            if isinstance(value, (bool, str)) or callable(value) or not np.isscalar(value) or not np.isreal(value):
                raise NotImplementedError(f"{type(self).__name__}: {self.SPELLINGS[key]} must be a number (arrays, fields and functions are "
                                          "not implemented)")
            values[key] = float(value)
        for key, value in values.items():
            setattr(self, key, value)

    def __getattr__(self, name):  # the reference's field names: mixing_length.Cˢ, getattr(equation, "Cᵂu★")
        key = type(self).canonical(name) if not name.startswith("_") else None
        if key is None or key == name:
            raise AttributeError(name)
        return getattr(self, key)


class CATKEMixingLength(_Coefficients):
    """CATKEMixingLength(; Cˢ = 1.131, Cᵇ = 0.28, Cˢᵖ = 0.505, CRiᵟ = 1.02, CRi⁰ = 0.254, Cʰⁱu = 0.242, Cˡᵒu = 0.361, Cᵘⁿu = 0.370, Cᶜu = 3.705,
    Cᵉu = 0, Cʰⁱc = 0.098, Cˡᵒc = 0.369, Cᵘⁿc = 0.572, Cᶜc = 4.793, Cᵉc = 0.112, Cʰⁱe = 0.548, Cˡᵒe = 7.863, Cᵘⁿe = 1.447, Cᶜe = 3.642, Cᵉe = 0)
    (catke_mixing_length.jl:15-36).  ASCII: C_s, C_b, C_sp, CRi_delta, CRi_0, C_hi_u, C_lo_u, C_un_u, C_c_u, C_e_u, ... _c, ... _e."""
    DEFAULTS = {"C_s": 1.131, "C_b": 0.28, "C_sp": 0.505, "CRi_delta": 1.02, "CRi_0": 0.254,
                "C_hi_u": 0.242, "C_lo_u": 0.361, "C_un_u": 0.370, "C_c_u": 3.705, "C_e_u": 0.0,
                "C_hi_c": 0.098, "C_lo_c": 0.369, "C_un_c": 0.572, "C_c_c": 4.793, "C_e_c": 0.112,
                "C_hi_e": 0.548, "C_lo_e": 7.863, "C_un_e": 1.447, "C_c_e": 3.642, "C_e_e": 0.0}
    SPELLINGS = {"C_s": "Cˢ", "C_b": "Cᵇ", "C_sp": "Cˢᵖ", "CRi_delta": "CRiᵟ", "CRi_0": "CRi⁰",
                 **{f"C_{a}_{x}": f"C{s}{x}" for x in "uce" for a, s in (("hi", "ʰⁱ"), ("lo", "ˡᵒ"), ("un", "ᵘⁿ"), ("c", "ᶜ"), ("e", "ᵉ"))}}


class CATKEEquation(_Coefficients):
    """CATKEEquation(; CʰⁱD = 0.579, CˡᵒD = 1.604, CᵘⁿD = 0.923, CᶜD = 3.254, CᵉD = 0, Cᵂu★ = 3.179, CᵂwΔ = 0.383, Cᵂϵ = 1)
    (catke_equation.jl:7-16).  ASCII: C_hi_D, C_lo_D, C_un_D, C_c_D, C_e_D, C_W_ustar, C_W_wdelta, C_W_eps."""
    DEFAULTS = {"C_hi_D": 0.579, "C_lo_D": 1.604, "C_un_D": 0.923, "C_c_D": 3.254, "C_e_D": 0.0, "C_W_ustar": 3.179, "C_W_wdelta": 0.383,
                "C_W_eps": 1.0}
    SPELLINGS = {"C_hi_D": "CʰⁱD", "C_lo_D": "CˡᵒD", "C_un_D": "CᵘⁿD", "C_c_D": "CᶜD", "C_e_D": "CᵉD", "C_W_ustar": "Cᵂu★", "C_W_wdelta": "CᵂwΔ",
                 "C_W_eps": "Cᵂϵ"}


class CATKEVerticalDiffusivity:
    """CATKEVerticalDiffusivity([time_discretization = VerticallyImplicitTimeDiscretization()]; mixing_length = CATKEMixingLength(),
    turbulent_kinetic_energy_equation = CATKEEquation(), maximum_tracer_diffusivity = Inf, maximum_tke_diffusivity = Inf,
    maximum_viscosity = Inf, minimum_tke = 1e-9, minimum_convective_buoyancy_flux = 1e-11, negative_tke_damping_time_scale = 1minute,
    tke_time_step = nothing) (catke_vertical_diffusivity.jl:96-120): κᵘ, κᶜ, κᵉ from a prognostic turbulent kinetic energy, the tracer "e",
    which the closure steps itself.  HydrostaticFreeSurfaceModel only; the explicit discretization, arrays of closures (ensembles) and
    coefficients that are no numbers are not implemented."""
    NUMBERS = {"maximum_tracer_diffusivity": math.inf, "maximum_tke_diffusivity": math.inf, "maximum_viscosity": math.inf, "minimum_tke": 1e-9,
               "minimum_convective_buoyancy_flux": 1e-11, "negative_tke_damping_time_scale": 60.0}
    MISSING_TRACER = "Tracers must contain :e to represent turbulent kinetic energy for `CATKEVerticalDiffusivity`."

    def __init__(self, *args, **kw):
        if len(args) > 1:
            raise TypeError("CATKEVerticalDiffusivity takes one positional argument, the time discretization")
        if args:
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"] = args[0]
        self.time_discretization = as_time_discretization(kw.pop("time_discretization", VerticallyImplicitTimeDiscretization()))
        if not isinstance(self.time_discretization, VerticallyImplicitTimeDiscretization):
            raise NotImplementedError("CATKEVerticalDiffusivity with ExplicitTimeDiscretization is not implemented: use the default "
                                      "VerticallyImplicitTimeDiscretization()")
        mixing_length = kw.pop("mixing_length", None)
        equation = kw.pop("turbulent_kinetic_energy_equation", None)
        self.mixing_length = CATKEMixingLength() if mixing_length is None else mixing_length
        self.turbulent_kinetic_energy_equation = CATKEEquation() if equation is None else equation
        if not isinstance(self.mixing_length, CATKEMixingLength):
            raise TypeError("mixing_length must be CATKEMixingLength(...)")
        if not isinstance(self.turbulent_kinetic_energy_equation, CATKEEquation):
            raise TypeError("turbulent_kinetic_energy_equation must be CATKEEquation(...)")
        for key, default in self.NUMBERS.items():
            value = kw.pop(key, default)
            if isinstance(value, (bool, str)) or callable(value) or not np.isscalar(value) or not np.isreal(value):
                raise NotImplementedError(f"CATKEVerticalDiffusivity: {key} must be a number (arrays, fields and functions are not implemented)")
            setattr(self, key, float(value))
        tke_time_step = kw.pop("tke_time_step", None)
        if tke_time_step is not None:
            if isinstance(tke_time_step, (bool, str)) or not np.isscalar(tke_time_step) or not np.isreal(tke_time_step) or not tke_time_step > 0:
                raise ValueError("tke_time_step must be None or a positive number")
            tke_time_step = float(tke_time_step)
        self.tke_time_step = tke_time_step
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")

    def c_struct(self):
        """struct ocn_catke"""
        ml, eq = self.mixing_length, self.turbulent_kinetic_energy_equation
        source = {**{k: getattr(ml, k) for k in ml.DEFAULTS}, **{k: getattr(eq, k) for k in eq.DEFAULTS}, **{k: getattr(self, k) for k in self.NUMBERS}}
        return _lib.CCatke(*[source[name] for name in _lib.CATKE_FIELDS])

    def __repr__(self):  # Base.summary (catke_vertical_diffusivity.jl:334-337)
        return f"CATKEVerticalDiffusivity{{{type(self.time_discretization).__name__}}}"


class TKEDissipationEquations(_Coefficients):
    """TKEDissipationEquations(; Cᵋϵ = 1.92, Cᴾϵ = 1.44, Cᵇϵ⁺ = -0.65, Cᵇϵ⁻ = -0.65, Cᵂu★ = 0, CᵂwΔ = 0, Cᵂα = 0.11, gravitational_acceleration =
    9.8065, minimum_roughness_length = 1e-4) (tke_dissipation_equations.jl:10-20).  ASCII: C_eps_eps, C_P_eps, C_b_eps_plus, C_b_eps_minus,
    C_W_ustar, C_W_wdelta, C_W_alpha."""
    DEFAULTS = {"C_eps_eps": 1.92, "C_P_eps": 1.44, "C_b_eps_plus": -0.65, "C_b_eps_minus": -0.65, "C_W_ustar": 0.0, "C_W_wdelta": 0.0,
                "C_W_alpha": 0.11, "gravitational_acceleration": 9.8065, "minimum_roughness_length": 1e-4}
    SPELLINGS = {"C_eps_eps": "Cᵋϵ", "C_P_eps": "Cᴾϵ", "C_b_eps_plus": "Cᵇϵ⁺", "C_b_eps_minus": "Cᵇϵ⁻", "C_W_ustar": "Cᵂu★", "C_W_wdelta": "CᵂwΔ",
                 "C_W_alpha": "Cᵂα", "gravitational_acceleration": "gravitational_acceleration",
                 "minimum_roughness_length": "minimum_roughness_length"}


class ConstantStabilityFunctions(_Coefficients):
    """ConstantStabilityFunctions(; Cσe = 1.0, Cσϵ = 1.2, Cu₀ = 0.53, Cc₀ = 0.53, 𝕊u₀ = 0.53) (tke_dissipation_stability_functions.jl:17-23): 𝕊u = Cu₀,
    𝕊c = Cc₀, 𝕊e = 𝕊u / Cσe, 𝕊ϵ = 𝕊u / Cσϵ.  ASCII: C_sigma_e, C_sigma_eps, Cu0, Cc0, Su0."""
    DEFAULTS = {"C_sigma_e": 1.0, "C_sigma_eps": 1.2, "Cu0": 0.53, "Cc0": 0.53, "Su0": 0.53}
    SPELLINGS = {"C_sigma_e": "Cσe", "C_sigma_eps": "Cσϵ", "Cu0": "Cu₀", "Cc0": "Cc₀", "Su0": "𝕊u₀"}
    CODE = _lib.STABILITY_CONSTANT

    def minimum_stratification_number(self, safety_factor):
        """(not read: the constants take no αᴺ)"""
        return 0.0

    def __repr__(self):  # Base.summary
        return "ConstantStabilityFunctions{Float64}"


class VariableStabilityFunctions(_Coefficients):
    """VariableStabilityFunctions(; Cσe = 1.0, Cσϵ = 1.2, Cu₀ = 0.1067, Cu₁ = 0.0173, Cu₂ = -0.0001205, Cc₀ = 0.1120, Cc₁ = 0.003766, Cc₂ = 0.0008871,
    Cd₀ = 1.0, Cd₁ = 0.2398, Cd₂ = 0.02872, Cd₃ = 0.005154, Cd₄ = 0.006930, Cd₅ = -0.0003372, 𝕊u₀ = nothing)
    (tke_dissipation_stability_functions.jl:40-100): 𝕊u and 𝕊c are rational functions of the clamped stratification and shear numbers.
    𝕊u₀ = nothing: the value of the logarithmic boundary layer, (2a / (-b - sqrt(b² - 4ac)))^(1/4) with a = Cd₅ - Cu₂, b = Cd₂ - Cu₀, c = Cd₀.
    ASCII: C_sigma_e, C_sigma_eps, Cu0 .. Cu2, Cc0 .. Cc2, Cd0 .. Cd5, Su0."""
    DEFAULTS = {"C_sigma_e": 1.0, "C_sigma_eps": 1.2, "Cu0": 0.1067, "Cu1": 0.0173, "Cu2": -0.0001205, "Cc0": 0.1120, "Cc1": 0.003766,
                "Cc2": 0.0008871, "Cd0": 1.0, "Cd1": 0.2398, "Cd2": 0.02872, "Cd3": 0.005154, "Cd4": 0.006930, "Cd5": -0.0003372, "Su0": None}
    SPELLINGS = {"C_sigma_e": "Cσe", "C_sigma_eps": "Cσϵ", "Su0": "𝕊u₀",
                 **{f"C{x}{n}": f"C{x}{s}" for x, count in (("u", 3), ("c", 3), ("d", 6)) for n, s in list(enumerate("₀₁₂₃₄₅"))[:count]}}
    CODE = _lib.STABILITY_VARIABLE

    def __init__(self, **kw):
        given = {name: value for name, value in kw.items() if not (self.canonical(name) == "Su0" and value is None)}
        super().__init__(**given)
        if self.Su0 is None:
            a, b, c = self.Cd5 - self.Cu2, self.Cd2 - self.Cu0, self.Cd0
            self.Su0 = (2 * a / (-b - math.sqrt(b * b - 4 * a * c))) ** (1 / 4)

    def minimum_stratification_number(self, safety_factor):
        """minimum_stratification_number(closure) (:150-173, Umlauf & Burchard 2005, eq. A.22), reduced by the safety factor"""
        a, b, c = self.Cd4 + self.Cc1, self.Cd1 + self.Cc0, self.Cd0
        return (-b + math.sqrt(b * b - 4 * a * c)) / (2 * a) * safety_factor

    def __repr__(self):  # Base.summary
        return "VariableStabilityFunctions{Float64}"


class StratifiedDisplacementScale(_Coefficients):
    """StratifiedDisplacementScale(; Cᴺ = 0.75, minimum_buoyancy_frequency = 1e-14) (tke_dissipation_vertical_diffusivity.jl:143-146): the floor
    of the dissipation, ϵ ≥ 𝕊u₀³ sqrt(e)³ / min(Lz, Cᴺ sqrt(e / N²)).  ASCII: C_N."""
    DEFAULTS = {"C_N": 0.75, "minimum_buoyancy_frequency": 1e-14}
    SPELLINGS = {"C_N": "Cᴺ", "minimum_buoyancy_frequency": "minimum_buoyancy_frequency"}


class TKEDissipationVerticalDiffusivity:
    """TKEDissipationVerticalDiffusivity([time_discretization = VerticallyImplicitTimeDiscretization()]; tke_dissipation_equations =
    TKEDissipationEquations(), stability_functions = VariableStabilityFunctions(), minimum_length_scale = StratifiedDisplacementScale(),
    maximum_tracer_diffusivity = Inf, maximum_tke_diffusivity = Inf, maximum_dissipation_diffusivity = Inf, maximum_viscosity = Inf,
    minimum_tke = 1e-6, minimum_stratification_number_safety_factor = 0.73, negative_tke_damping_time_scale = 1minute,
    tke_dissipation_time_step = nothing) (tke_dissipation_vertical_diffusivity.jl:102-129): the k-ϵ closure (Burchard & Bolding 2001, Umlauf &
    Burchard 2003, 2005).  κᵘ, κᶜ, κᵉ, κᵋ = 𝕊 e² / ϵ from two prognostic tracers, the turbulent kinetic energy "e" and its dissipation
    ("epsilon", "ϵ" or "ε"), which the closure steps itself.  HydrostaticFreeSurfaceModel only; the explicit discretization, arrays of closures
    (ensembles) and coefficients that are no numbers are not implemented."""
    NUMBERS = {"maximum_tracer_diffusivity": math.inf, "maximum_tke_diffusivity": math.inf, "maximum_dissipation_diffusivity": math.inf,
               "maximum_viscosity": math.inf, "minimum_tke": 1e-6, "minimum_stratification_number_safety_factor": 0.73,
               "negative_tke_damping_time_scale": 60.0}
    MISSING_TRACER = "Tracers must contain :e and :ϵ to represent turbulent kinetic energy for `TKEDissipationVerticalDiffusivity`."
    DISSIPATION_NAMES = ("epsilon", "ϵ", "ε")  # canonical, the reference's (U+03F5), the Greek letter (U+03B5)
    PARTS = {"tke_dissipation_equations": (TKEDissipationEquations,), "stability_functions": (VariableStabilityFunctions, ConstantStabilityFunctions),
             "minimum_length_scale": (StratifiedDisplacementScale,)}

    def __init__(self, *args, **kw):
        if len(args) > 1:
            raise TypeError("TKEDissipationVerticalDiffusivity takes one positional argument, the time discretization")
        if args:
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"] = args[0]
        self.time_discretization = as_time_discretization(kw.pop("time_discretization", VerticallyImplicitTimeDiscretization()))
        if not isinstance(self.time_discretization, VerticallyImplicitTimeDiscretization):
            raise NotImplementedError("TKEDissipationVerticalDiffusivity with ExplicitTimeDiscretization is not implemented: use the default "
                                      "VerticallyImplicitTimeDiscretization()")
        for key, kinds in self.PARTS.items():
            part = kw.pop(key, None)
            part = kinds[0]() if part is None else part
            if not isinstance(part, kinds):
                raise TypeError(f"{key} must be " + " or ".join(f"{kind.__name__}(...)" for kind in kinds))
            setattr(self, key, part)
        for key, default in self.NUMBERS.items():
            value = kw.pop(key, default)
            if isinstance(value, (bool, str)) or callable(value) or not np.isscalar(value) or not np.isreal(value):
                raise NotImplementedError(f"TKEDissipationVerticalDiffusivity: {key} must be a number (arrays, fields and functions are not "
                                          "implemented)")
            setattr(self, key, float(value))
        time_step = kw.pop("tke_dissipation_time_step", None)
        if time_step is not None:
            if isinstance(time_step, (bool, str)) or not np.isscalar(time_step) or not np.isreal(time_step) or not time_step > 0:
                raise ValueError("tke_dissipation_time_step must be None or a positive number")
            time_step = float(time_step)
        self.tke_dissipation_time_step = time_step
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")

    @classmethod
    def dissipation_name(cls, tracers):
        """the name the user gave the dissipation tracer, or None"""
        return next((name for name in cls.DISSIPATION_NAMES if name in tuple(tracers)), None)

    def derived_constants(self):
        """what depends on the coefficients alone, in Python floats: the kernels and the tests' restatement take these bits.  𝕊u₀⁴ is
        (𝕊u₀ 𝕊u₀) (𝕊u₀ 𝕊u₀)"""
        sf = self.stability_functions
        Su0 = sf.Su0
        return {"Su0": Su0, "Su0_cubed": Su0 * Su0 * Su0, "Su0_fourth_over_sigma_eps": (Su0 * Su0) * (Su0 * Su0) / sf.C_sigma_eps,
                "minimum_stratification_number": sf.minimum_stratification_number(self.minimum_stratification_number_safety_factor)}

    def c_struct(self):
        """struct ocn_tke_dissipation"""
        eq, sf, ls = self.tke_dissipation_equations, self.stability_functions, self.minimum_length_scale
        source = {name: 0.0 for name in _lib.TKE_DISSIPATION_FIELDS}  # (the coefficients that ConstantStabilityFunctions does not have)
        for part in (eq, sf, ls):
            source.update({k: getattr(part, k) for k in part.DEFAULTS})
        source.update({k: getattr(self, k) for k in self.NUMBERS if k in source})
        source.update(self.derived_constants())
        return _lib.CTKEDissipation(*[source[name] for name in _lib.TKE_DISSIPATION_FIELDS], sf.CODE, 0)

    def __repr__(self):  # Base.summary (tke_dissipation_vertical_diffusivity.jl:363-366)
        return f"TKEDissipationVerticalDiffusivity{{{type(self.time_discretization).__name__}}}"


def has_diffusivity_fields(closure):
    """closures of the VerticalFormulation whose κᶜ, κᵘ are (Center, Center, Face) fields that the HydrostaticFreeSurfaceModel computes in
    update_state! (their term and implicit step: csrc/vertical_diffusivity.hip)"""
    return isinstance(closure, (ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity, CATKEVerticalDiffusivity,
                                TKEDissipationVerticalDiffusivity))


class AdvectiveFormulation:
    """AdvectiveFormulation() (isopycnal_skew_symmetric_diffusivity.jl:3): the skew flux as advection by the eddy velocities"""

    def __repr__(self):
        return type(self).__name__ + "()"


class DiffusiveFormulation:
    """DiffusiveFormulation() (:4): the skew flux as the antisymmetric part of the diffusion tensor"""

    def __repr__(self):
        return type(self).__name__ + "()"


class SmallSlopeIsopycnalTensor:
    """SmallSlopeIsopycnalTensor(; minimum_bz = 0) (isopycnal_rotation_tensor_components.jl:60-64)"""

    def __init__(self, minimum_bz=0.0):
        if isinstance(minimum_bz, (bool, str)) or not np.isscalar(minimum_bz) or not np.isreal(minimum_bz) or math.isnan(minimum_bz):
            raise ValueError("minimum_bz must be a number")
        self.minimum_bz = float(minimum_bz)

    def __repr__(self):
        return f"{type(self).__name__}{{Float64}}({_prettysummary(self.minimum_bz, compact=False)})"


class IsopycnalTensor(SmallSlopeIsopycnalTensor):
    """IsopycnalTensor(minimum_bz) (:28-30): constructible; IsopycnalSkewSymmetricDiffusivity refuses it, as the reference does"""

    def __init__(self, minimum_bz):
        super().__init__(minimum_bz)


class FluxTapering:
    """FluxTapering(max_slope) (isopycnal_skew_symmetric_diffusivity.jl:149-151): every flux is scaled by min(1, max_slope² / slope²)"""

    def __init__(self, max_slope):
        if isinstance(max_slope, (bool, str)) or not np.isscalar(max_slope) or not np.isreal(max_slope):
            raise NotImplementedError("FluxTapering: max_slope must be a number")
        if not (math.isfinite(max_slope) and max_slope > 0):
            raise ValueError("FluxTapering: max_slope must be finite and positive")
        self.max_slope = float(max_slope)

    def __repr__(self):
        return f"FluxTapering{{Float64}}({_prettysummary(self.max_slope, compact=False)})"


class IsopycnalSkewSymmetricDiffusivity:
    """IsopycnalSkewSymmetricDiffusivity([time_discretization = VerticallyImplicitTimeDiscretization()]; κ_skew = nothing, κ_symmetric = nothing,
    skew_flux_formulation = AdvectiveFormulation(), isopycnal_tensor = SmallSlopeIsopycnalTensor(), slope_limiter = FluxTapering(1e-2),
    required_halo_size = 1) (isopycnal_skew_symmetric_diffusivity.jl:50-71): Gent-McWilliams skew transport with κ_skew and Redi diffusion
    along isopycnals with κ_symmetric (csrc/isopycnal.hip).  ASCII aliases: kappa_skew, kappa_symmetric.  The coefficients are numbers or None
    (the reference's nothing); κ_symmetric may be a dict {tracer name: κ}, κ_skew only with the DiffusiveFormulation.  The vertical part
    of the symmetric flux is stepped implicitly; HydrostaticFreeSurfaceModel only."""
    PER_TRACER_SKEW = "Only one skew coefficient for all tracers is currently supported with the AdvectiveFormulation."
    ONLY_SMALL_SLOPE = "Only isopycnal_tensor=SmallSlopeIsopycnalTensor() is currently supported."

    def __init__(self, *args, **kw):
        if len(args) > 1:
            raise TypeError("IsopycnalSkewSymmetricDiffusivity takes one positional argument, the time discretization")
        if args:
            if "time_discretization" in kw:
                raise TypeError("time_discretization given twice")
            kw["time_discretization"] = args[0]
        self.time_discretization = as_time_discretization(kw.pop("time_discretization", VerticallyImplicitTimeDiscretization()))
        if not isinstance(self.time_discretization, VerticallyImplicitTimeDiscretization):
            raise NotImplementedError("IsopycnalSkewSymmetricDiffusivity with the ExplicitTimeDiscretization is not implemented: the reference's own "
                                      "explicit method cannot be called (the call of explicit_κ_∂z_c in diffusive_flux_z, "
                                      "isopycnal_skew_symmetric_diffusivity.jl:308, does not match the method at :316); use the default, "
                                      "VerticallyImplicitTimeDiscretization()")
        for greek, ascii_name in (("κ_skew", "kappa_skew"), ("κ_symmetric", "kappa_symmetric")):
            if greek in kw and ascii_name in kw:
                raise TypeError(f"{greek} given twice")
        kappa_skew = kw.pop("κ_skew", kw.pop("kappa_skew", None))
        kappa_symmetric = kw.pop("κ_symmetric", kw.pop("kappa_symmetric", None))
        formulation = kw.pop("skew_flux_formulation", None)
        formulation = AdvectiveFormulation() if formulation is None else (formulation() if isinstance(formulation, type) else formulation)
        if not isinstance(formulation, (AdvectiveFormulation, DiffusiveFormulation)):
            raise TypeError("skew_flux_formulation must be AdvectiveFormulation() or DiffusiveFormulation()")
        tensor = kw.pop("isopycnal_tensor", None)
        tensor = SmallSlopeIsopycnalTensor() if tensor is None else tensor
        limiter = kw.pop("slope_limiter", None)
        limiter = FluxTapering(1e-2) if limiter is None else limiter
        halo = kw.pop("required_halo_size", 1)
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
        self.advective = isinstance(formulation, AdvectiveFormulation)
        if isinstance(kappa_skew, dict) and self.advective:
            raise ValueError(self.PER_TRACER_SKEW)
        if type(tensor) is not SmallSlopeIsopycnalTensor:
            raise NotImplementedError(self.ONLY_SMALL_SLOPE)
        if not isinstance(limiter, FluxTapering):
            raise NotImplementedError("IsopycnalSkewSymmetricDiffusivity: slope_limiter must be FluxTapering(max_slope)")
        if isinstance(halo, bool) or not isinstance(halo, (int, np.integer)) or halo < 1:
            raise ValueError("required_halo_size must be an integer >= 1")

        def number(x, what):
            if isinstance(x, (bool, str)) or callable(x) or not np.isscalar(x) or not np.isreal(x):
                raise NotImplementedError(f"IsopycnalSkewSymmetricDiffusivity: {what} must be a number (functions, arrays and fields are not "
                                          "implemented)")
            return float(x)  # convert_diffusivity(FT, κ)

        def coefficient(x, what):
            if x is None:
                return None
            if isinstance(x, dict):
                return {str(k): number(v, f"{what} of {k}") for k, v in x.items()}
            return number(x, what)
        self.kappa_skew = coefficient(kappa_skew, "κ_skew")
        self.kappa_symmetric = coefficient(kappa_symmetric, "κ_symmetric")
        self.skew_flux_formulation, self.isopycnal_tensor, self.slope_limiter = formulation, tensor, limiter
        self.required_halo_size = int(halo)

    κ_skew = property(lambda self: self.kappa_skew)
    κ_symmetric = property(lambda self: self.kappa_symmetric)

    @staticmethod
    def _of(kappa, name):
        """get_tracer_κ (:220-222): nothing is 0"""
        if kappa is None:
            return 0.0
        if isinstance(kappa, dict):
            if name not in kappa:
                raise ValueError(f"no diffusivity κ given for tracer {name}")
            return kappa[name]
        return kappa

    def kappa_symmetric_of(self, name):
        return self._of(self.kappa_symmetric, name)

    def kappa_skew_of(self, name):
        """the skew coefficient inside the diffusive fluxes: 0 with the AdvectiveFormulation (skew_diffusivity, :225-226)"""
        return 0.0 if self.advective else self._of(self.kappa_skew, name)

    def c_struct(self):
        """struct ocn_isopycnal"""
        return _lib.CIsopycnal(self.slope_limiter.max_slope, self.isopycnal_tensor.minimum_bz)

    @staticmethod
    def _shown(kappa, pretty):
        if kappa is None:
            return "Nothing" if pretty else "nothing"
        if isinstance(kappa, dict):
            sep = "=" if pretty else " = "
            items = [f"{k}{sep}{_prettysummary(v, compact=pretty)}" for k, v in kappa.items()]
            return "(" + ", ".join(items) + ("," if len(items) == 1 else "") + ")" if items else "NamedTuple()"
        return _prettysummary(kappa, compact=pretty)

    def summary(self):  # Base.summary (:350-353)
        return f"IsopycnalSkewSymmetricDiffusivity(κ_skew={self._shown(self.kappa_skew, True)}, κ_symmetric={self._shown(self.kappa_symmetric, True)})"

    def __repr__(self):  # Base.show (:355-358)
        return (f"IsopycnalSkewSymmetricDiffusivity: (κ_symmetric={self._shown(self.kappa_symmetric, False)}, "
                f"κ_skew={self._shown(self.kappa_skew, False)}, (isopycnal_tensor={self.isopycnal_tensor!r}, slope_limiter={self.slope_limiter!r})")


class ThreeDimensionalFormulation:
    """ThreeDimensionalFormulation() (TurbulenceClosures.jl): the closure acts isotropically"""

    def __repr__(self):
        return type(self).__name__ + "()"


class HorizontalFormulation(ThreeDimensionalFormulation):
    """HorizontalFormulation(): the closure acts in x and y"""


class VerticalFormulation(ThreeDimensionalFormulation):
    """VerticalFormulation(): the closure acts in z"""


class HorizontalDivergenceFormulation(ThreeDimensionalFormulation):
    """HorizontalDivergenceFormulation(): the closure acts on the horizontal divergence alone"""


_FORMULATIONS = (ThreeDimensionalFormulation, HorizontalFormulation, VerticalFormulation, HorizontalDivergenceFormulation)


def as_formulation(formulation):
    """an instance, a class, or one of the strings "ThreeDimensional" / "Horizontal" / "Vertical" / "HorizontalDivergence" (with or
    without "Formulation") -> an instance"""
    if isinstance(formulation, _FORMULATIONS):
        return formulation
    for F in _FORMULATIONS:
        if formulation is F or formulation in (F.__name__, F.__name__[:-len("Formulation")]):
            return F()
    raise ValueError(f"formulation must be one of {', '.join(F.__name__ + '()' for F in _FORMULATIONS)}, got {formulation!r}")


class ScalarBiharmonicDiffusivity:
    """ScalarBiharmonicDiffusivity(formulation = ThreeDimensionalFormulation(); ν = 0, κ = 0) (scalar_biharmonic_diffusivity.jl:75-95):
    a hyperviscosity ν ∇⁴ and hyperdiffusivity κ ∇⁴, always explicit in time (abstract_scalar_biharmonic_diffusivity_closure.jl:8).
    Only the HorizontalFormulation with constant coefficients is implemented (HorizontalScalarBiharmonicDiffusivity: csrc/biharmonic.hip;
    HydrostaticFreeSurfaceModel on a grid Periodic in x and y); every other formulation, and function / array / field coefficients,
    discrete_form, loc, parameters and a required_halo_size other than 2 raise NotImplementedError.
    κ is a number (every tracer) or a dict {tracer name: κ}.  ASCII aliases: nu, kappa.  `formulation` is an instance or a string
    ("Horizontal", ...)."""
    required_halo_size = 2

    def __init__(self, formulation="ThreeDimensional", **kw):
        self.formulation = as_formulation(formulation)
        name = type(self.formulation).__name__
        if type(self.formulation) is not HorizontalFormulation:
            raise NotImplementedError(f"ScalarBiharmonicDiffusivity: the {name} is not implemented, only the HorizontalFormulation "
                                      "(HorizontalScalarBiharmonicDiffusivity; see DESIGN.md §5.2l)")
        for greek, ascii_name in (("ν", "nu"), ("κ", "kappa")):
            if greek in kw and ascii_name in kw:
                raise TypeError(f"{greek} given twice")
        nu = kw.pop("ν", kw.pop("nu", 0.0))
        kappa = kw.pop("κ", kw.pop("kappa", 0.0))
        if kw.pop("discrete_form", False):
            raise NotImplementedError("ScalarBiharmonicDiffusivity: discrete_form = true is not implemented (constant ν, κ only)")
        if kw.pop("loc", None) not in (None, (None, None, None)):
            raise NotImplementedError("ScalarBiharmonicDiffusivity: loc is not implemented (constant ν, κ only)")
        if kw.pop("parameters", None) is not None:
            raise NotImplementedError("ScalarBiharmonicDiffusivity: parameters is not implemented (constant ν, κ only)")
        if kw.pop("required_halo_size", 2) != 2:
            raise NotImplementedError("ScalarBiharmonicDiffusivity: a required_halo_size other than 2 is not implemented (it serves "
                                      "coefficient functions; constant ν, κ need 2)")
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")

        def number(x, what):
            if isinstance(x, (bool, str)) or callable(x) or not np.isscalar(x) or not np.isreal(x):
                raise NotImplementedError(f"ScalarBiharmonicDiffusivity: {what} must be a number (functions, arrays and fields are not "
                                          "implemented)")
            return x
        self._given_nu = number(nu, "ν")
        self.nu = float(nu)
        if isinstance(kappa, dict):
            self.kappa = {str(k): number(v, f"κ of {k}") for k, v in kappa.items()}
        else:
            self.kappa = number(kappa, "κ")
        self.time_discretization = ExplicitTimeDiscretization()

    ν = property(lambda self: self.nu)
    κ = property(lambda self: self.kappa)

    def kappa_of(self, name):
        if isinstance(self.kappa, dict):
            if name not in self.kappa:
                raise ValueError(f"no diffusivity κ given for tracer {name}")
            return float(self.kappa[name])
        return float(self.kappa)

    def __eq__(self, other):
        return (isinstance(other, ScalarBiharmonicDiffusivity) and type(other.formulation) is type(self.formulation)
                and other.nu == self.nu and other.kappa == self.kappa)

    __hash__ = None

    def __repr__(self):  # Base.summary (scalar_biharmonic_diffusivity.jl:105-115)
        if isinstance(self.kappa, dict):
            kappa = "(" + ", ".join(f"{k}={_prettysummary(v)}" for k, v in self.kappa.items()) + ("," if len(self.kappa) == 1 else "") + ")"
        else:
            kappa = _prettysummary(self.kappa)
        return f"ScalarBiharmonicDiffusivity{{{type(self.formulation).__name__}}}(ν={_prettysummary(self.nu)}, κ={kappa})"


def HorizontalScalarBiharmonicDiffusivity(**kw):
    """HorizontalScalarBiharmonicDiffusivity(; ν = 0, κ = 0) = ScalarBiharmonicDiffusivity(HorizontalFormulation(); ν, κ)
    (scalar_biharmonic_diffusivity.jl:18)"""
    return ScalarBiharmonicDiffusivity(HorizontalFormulation(), **kw)


class AnisotropicMinimumDissipation:
    """AnisotropicMinimumDissipation(; C = 1/12, Cν = nothing, Cκ = nothing, Cb = nothing)
    (anisotropic_minimum_dissipation.jl:106-115): ExplicitTimeDiscretization, number (or per-tracer dict) Poincaré constants."""

    def __init__(self, C=1 / 12, Cnu=None, Ckappa=None, Cb=None, **kw):
        Cnu = kw.pop("Cν", Cnu)
        Ckappa = kw.pop("Cκ", Ckappa)
        if kw:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
        if Cb is not None:
            raise NotImplementedError("the buoyancy modification (Cb) is not implemented")
        self.Cnu = float(C if Cnu is None else Cnu)
        self.Ckappa = C if Ckappa is None else Ckappa
        if callable(self.Ckappa) or callable(Cnu):
            raise NotImplementedError("only number Poincaré constants are implemented")

    def Ckappa_of(self, name):
        if isinstance(self.Ckappa, dict):
            if name not in self.Ckappa:
                raise ValueError(f"no Poincaré constant Cκ given for tracer {name}")
            return float(self.Ckappa[name])
        return float(self.Ckappa)


class LillyCoefficient:
    """LillyCoefficient(; smagorinsky = 0.16, reduction_factor = 1) (Smagorinskys/lilly_coefficient.jl:44-45): the Smagorinsky coefficient
    reduced by the stability function ς = sqrt(1 - min(1, Cb max(0, N²) / Σ²))."""

    def __init__(self, smagorinsky=0.16, reduction_factor=1):
        self.smagorinsky = float(smagorinsky)
        self.reduction_factor = float(reduction_factor)

    def __repr__(self):
        return f"LillyCoefficient(smagorinsky = {self.smagorinsky}, reduction_factor = {self.reduction_factor})"


class DynamicCoefficient:
    """DynamicCoefficient(; averaging, ...) (Smagorinskys/dynamic_coefficient.jl): not implemented."""

    def __init__(self, *args, **kw):
        raise NotImplementedError("DynamicCoefficient (the scale-invariant dynamic Smagorinsky procedure) is not implemented")


class Smagorinsky:
    """Smagorinsky(; coefficient = 0.16, Pr = 1.0) (Smagorinskys/smagorinsky.jl:75-81): νₑ = (Cˢ Δᶠ)² sqrt(2 Σ²), κₑ = νₑ / Pr.
    `coefficient` is a number or a LillyCoefficient; Pr is a number (every tracer) or a dict {tracer name: Pr}.
    ExplicitTimeDiscretization only."""

    def __init__(self, coefficient=0.16, Pr=1.0, time_discretization="Explicit"):
        if not isinstance(as_time_discretization(time_discretization), ExplicitTimeDiscretization):
            raise NotImplementedError("VerticallyImplicitTimeDiscretization is not implemented")
        if isinstance(coefficient, type) or callable(coefficient):
            raise NotImplementedError("only a number or a LillyCoefficient is implemented as the Smagorinsky coefficient")
        if not isinstance(coefficient, LillyCoefficient):
            if np.ndim(coefficient) > 0:
                raise NotImplementedError("only a number or a LillyCoefficient is implemented as the Smagorinsky coefficient")
            coefficient = float(coefficient)
        if callable(Pr) or (not isinstance(Pr, dict) and np.ndim(Pr) > 0):
            raise NotImplementedError("only number (or per-tracer dict) Prandtl numbers are implemented")
        self.coefficient = coefficient
        self.Pr = {k: float(v) for k, v in Pr.items()} if isinstance(Pr, dict) else float(Pr)

    @property
    def lilly(self):
        return isinstance(self.coefficient, LillyCoefficient)

    @property
    def C(self):
        return self.coefficient.smagorinsky if self.lilly else self.coefficient

    @property
    def Cb(self):
        return self.coefficient.reduction_factor if self.lilly else 0.0

    def Pr_of(self, name):
        if isinstance(self.Pr, dict):
            if name not in self.Pr:
                raise ValueError(f"no Prandtl number Pr given for tracer {name}")
            return self.Pr[name]
        return self.Pr

    def c_struct(self, tracer_names):
        """struct ocn_smagorinsky for these tracers"""
        s = _lib.CSmagorinsky()
        s.C, s.Cb, s.lilly, s.n_tracers = self.C, self.Cb, int(self.lilly), len(tracer_names)
        for n, name in enumerate(tracer_names):
            s.Pr[n] = self.Pr_of(name)
        return s

    def __repr__(self):
        return f"Smagorinsky(coefficient = {self.coefficient!r}, Pr = {self.Pr})"


def SmagorinskyLilly(C=0.16, Cb=1, Pr=1, time_discretization="Explicit"):
    """SmagorinskyLilly(; C = 0.16, Cb = 1, Pr = 1) = Smagorinsky(coefficient = LillyCoefficient(C, Cb), Pr = Pr) (lilly_coefficient.jl:106-111)"""
    return Smagorinsky(coefficient=LillyCoefficient(smagorinsky=C, reduction_factor=Cb), Pr=Pr, time_discretization=time_discretization)


def DynamicSmagorinsky(*args, **kw):
    """DynamicSmagorinsky(; averaging, Pr, ...) (Smagorinskys/dynamic_coefficient.jl): not implemented."""
    raise NotImplementedError("DynamicSmagorinsky is not implemented")


def owns_eddy_fields(closure):
    """closures whose diffusivity_fields hold a νₑ Center field (and κₑ fields) that compute_diffusivities fills"""
    return isinstance(closure, (AnisotropicMinimumDissipation, Smagorinsky))


class LinearEquationOfState:
    """linear_equation_of_state.jl:33-35"""

    def __init__(self, thermal_expansion=1.67e-4, haline_contraction=7.80e-4):
        self.thermal_expansion = float(thermal_expansion)
        self.haline_contraction = float(haline_contraction)


class BuoyancyTracer:
    required_tracers = ("b",)


class SeawaterBuoyancy:
    """seawater_buoyancy.jl:88-108; g_Earth = 9.80665 (BuoyancyFormulations.jl)"""

    def __init__(self, gravitational_acceleration=9.80665, equation_of_state=None, constant_temperature=None,
                 constant_salinity=None):
        eos = LinearEquationOfState() if equation_of_state is None else equation_of_state
        if not isinstance(eos, LinearEquationOfState):
            raise NotImplementedError("only LinearEquationOfState is implemented")
        if constant_temperature is not None and constant_salinity is not None:
            raise ValueError("constant_temperature and constant_salinity cannot both be set")
        self.equation_of_state = eos
        self.gravitational_acceleration = float(gravitational_acceleration)
        self.constant_temperature = constant_temperature
        self.constant_salinity = constant_salinity

    @property
    def required_tracers(self):
        if self.constant_salinity is not None:
            return ("T",)
        if self.constant_temperature is not None:
            return ("S",)
        return ("T", "S")


# --------------------------------------------------------------------------------------------------------
# Boundary conditions
# --------------------------------------------------------------------------------------------------------
class BoundaryCondition:
    """BoundaryCondition(classification, condition).  `condition` is a number, an array over the boundary's two tangential directions
    or a function of the tangential coordinates and time; `coeff` restates the
    ContinuousBoundaryFunction  f(x, y, t, c, p) = p * c  with field_dependencies = the field itself as
    condition + coeff * c[i, j, boundary-adjacent cell] (include/ocn_hip.h: struct ocn_bc)."""

    def __init__(self, kind, condition=0.0, coeff=0.0, parameters=None, field_dependencies=(), discrete_form=False):
        """field_dependencies (flux conditions only): a name or a tuple of names of velocities and tracers of the model; `condition` is then a
        function f(ξ, η, t, *dependencies[, parameters]) that is traced once and evaluated on the device (boundary_functions.py).
        condition: a number, an (Nx, Ny) array, or a function f(x, y, t) [f(x, y, t, parameters) with `parameters`] of the two
        coordinates tangential to a bottom / top boundary (without those of Flat directions: f(x, t) on an x-z slice) and time -- the reference's ContinuousBoundaryFunction without field
        dependencies (continuous_boundary_function.jl:17-115).  The function is evaluated on the host at the field's own nodes (called
        once with broadcastable arrays) every time the model state is updated, with the clock time of that moment, and uploaded into
        the (Nx, Ny) device array the kernels read."""
        if discrete_form:
            raise NotImplementedError("discrete_form=True: boundary functions f(i, j, grid, clock, model_fields) are not implemented -- the library is "
                                      "compiled ahead of time and takes no kernel functions (see DESIGN.md §5.2i)")
        field_dependencies = (field_dependencies,) if isinstance(field_dependencies, str) else tuple(field_dependencies)
        if field_dependencies:
            if kind != _lib.BC_FLUX:
                raise NotImplementedError("field_dependencies on a Value, Gradient or Open boundary condition are not implemented: those conditions "
                                          "are evaluated inside the halo fills, where the tangential halos of the other fields are not defined "
                                          "yet; FluxBoundaryCondition takes them (see DESIGN.md §5.2i)")
            if any(not isinstance(n, str) for n in field_dependencies):
                raise TypeError("field_dependencies must be a name or a tuple of names of model fields")
            if not callable(condition):
                raise TypeError("field_dependencies need a function f(ξ, η, t, *dependencies[, parameters]) as the condition")
            if coeff != 0.0:
                raise ValueError("coeff together with field_dependencies: name the field itself among the dependencies instead")
        self.field_dependencies = field_dependencies
        self.kind = kind
        self.coeff = float(coeff)
        self.values = None
        self.value = 0.0
        self.func, self.parameters = None, parameters
        if np.isscalar(condition):
            self.value = float(condition)
        elif callable(condition):
            self.func = condition
        else:
            self.values = np.ascontiguousarray(np.asarray(condition, dtype=np.float64).T)  # stored [j, i]: x fastest
        self._device_values = None

    # the two directions tangential to a side, in the order the kernels index `values` (first one fastest): csrc/kernels.hip
    # fill_halos_general_kernel / apply_flux_bcs_lateral_kernel / apply_flux_bcs_kernel -> values[(a1 - 1) + n1 (a2 - 1)]
    _TANGENTIAL = {"west": (1, 2), "east": (1, 2), "south": (0, 2), "north": (0, 2), "bottom": (0, 1), "top": (0, 1)}

    def _extents(self, grid, side):
        N = (grid.Nx, grid.Ny, grid.Nz)
        d1, d2 = self._TANGENTIAL[side]
        return N[d1], N[d2]

    def refresh(self, grid, loc, time, side="top"):
        """Re-evaluate a function-valued condition at `time` (no-op otherwise): f(ξ, η, t[, p]) of the two coordinates tangential to the
        boundary -- (x, y) on bottom / top, (y, z) on west / east, (x, z) on south / north -- at the field's own nodes there
        (continuous_boundary_function.jl:17-115: the reference's ContinuousBoundaryFunction without field dependencies)."""
        if self.func is None or self.field_dependencies:  # (a function of the model's fields is evaluated on the device: models.py)
            return
        d1, d2 = self._TANGENTIAL[side]
        n1, n2 = self._extents(grid, side)
        nodes = grid.nodes(loc)
        c1 = np.asarray(nodes[d1]).reshape(-1)[:n1].reshape(-1, 1)
        c2 = np.asarray(nodes[d2]).reshape(-1)[:n2].reshape(1, -1)
        # the coordinates of Flat directions are not arguments (a top condition on a (Bounded, Flat, Bounded) grid is f(x, t[, p]),
        # examples/horizontal_convection.jl:47)
        coords = tuple(c for c, d in zip((c1, c2), (d1, d2)) if grid.topology[d] != "Flat")
        args = coords + (float(time),) if self.parameters is None else coords + (float(time), self.parameters)
        vals = np.broadcast_to(np.asarray(self.func(*args), dtype=np.float64), (n1, n2))
        self.values = np.array(vals.T, dtype=np.float64, order="C")  # (a copy: broadcast views are read-only)
        if self._device_values is None:
            self._device_values = on_architecture(grid.architecture, self.values)
        else:
            import torch
            self._device_values.copy_(torch.from_numpy(self.values))

    def c_struct(self, grid, side="top"):
        ptr = None
        if self.func is not None and self._device_values is None:
            raise RuntimeError("function-valued boundary condition used before its first evaluation (update_boundary_conditions)")
        if self.values is not None:
            n1, n2 = self._extents(grid, side)
            if self.values.shape != (n2, n1):
                raise ValueError(f"array boundary condition on the {side} boundary has shape {self.values.T.shape}, expected {(n1, n2)}")
            if self._device_values is None:
                self._device_values = on_architecture(grid.architecture, self.values)
            ptr = self._device_values.data_ptr()
        elif self.field_dependencies:  # the array ocn_op_compute_boundary writes (boundary_functions.BoundaryFunction)
            ptr = self._device_values.data_ptr()
        return _lib.CBc(self.kind, 0, self.value, self.coeff, ptr)


def FluxBoundaryCondition(condition=0.0, coeff=0.0, parameters=None, field_dependencies=(), discrete_form=False):
    """FluxBoundaryCondition(condition; parameters, field_dependencies): with field_dependencies = a name or a tuple of names of velocities
    and tracers, `condition` is the reference's f(ξ, η, t, *dependencies[, parameters]) -- quadratic drag is
    lambda x, y, t, u, v, p: -p["cd"] * ocn.sqrt(u ** 2 + v ** 2) * u -- traced once and evaluated on the device at every tendency evaluation"""
    return BoundaryCondition(_lib.BC_FLUX, condition, coeff, parameters, field_dependencies, discrete_form)


def ValueBoundaryCondition(condition=0.0, parameters=None, field_dependencies=(), discrete_form=False):
    return BoundaryCondition(_lib.BC_VALUE, condition, parameters=parameters, field_dependencies=field_dependencies, discrete_form=discrete_form)


def GradientBoundaryCondition(condition=0.0, parameters=None, field_dependencies=(), discrete_form=False):
    return BoundaryCondition(_lib.BC_GRADIENT, condition, parameters=parameters, field_dependencies=field_dependencies,
                             discrete_form=discrete_form)


def OpenBoundaryCondition(condition=0.0, parameters=None, field_dependencies=(), discrete_form=False):
    """OpenBoundaryCondition(value) on the side a velocity component is normal to: that component ON the boundary face is set to the
    value (a number, an array over the tangential directions or a function of the tangential coordinates and time) by every halo fill
    that fills boundary-normal velocities (fill_halo_regions_open.jl:9-70); the default Impenetrable condition is Open(nothing) = 0."""
    return BoundaryCondition(_lib.BC_OPEN, condition, parameters=parameters, field_dependencies=field_dependencies, discrete_form=discrete_form)


class FieldBoundaryConditions:
    """FieldBoundaryConditions(; west, east, south, north, bottom, top); unspecified sides keep the topology defaults
    (field_boundary_conditions.jl:15-33).  Flux, Value, Gradient on every side of a Bounded direction, each a number, condition +
    coeff * c, an array over the two tangential directions ((Ny, Nz) on west / east, (Nx, Nz) on south / north, (Nx, Ny) on bottom /
    top) or a function of the tangential coordinates and time; the fluxes of the lateral sides enter through apply_x_bcs! /
    apply_y_bcs! (apply_flux_bcs.jl:38-146)."""
    SIDES = ("west", "east", "south", "north", "bottom", "top")

    def __init__(self, **sides):
        for k in sides:
            if k == "immersed":
                raise NotImplementedError("immersed = ... boundary conditions are not implemented: an immersed boundary is no-flux for tracers "
                                          "and free-slip for momentum (leave `immersed` out)")
            if k not in self.SIDES:
                raise TypeError(f"unknown boundary {k!r}")
        self.sides = {k: sides.get(k) for k in self.SIDES}
        self._c = None

    def is_default(self):
        return all(v is None for v in self.sides.values())

    def refresh(self, grid, loc, time):
        """update_boundary_condition! for function-valued conditions: evaluate them at the clock time"""
        for k, v in self.sides.items():
            if v is not None:
                v.refresh(grid, loc, time, k)

    def has_flux(self):
        return any(v is not None and v.kind == _lib.BC_FLUX for v in self.sides.values())

    def field_dependent(self):
        """(side, condition) of the conditions that are functions of the model's fields"""
        return [(k, v) for k, v in self.sides.items() if v is not None and v.field_dependencies]

    def c_struct(self, grid):
        if self._c is None:
            default = _lib.CBc(_lib.BC_DEFAULT, 0, 0.0, 0.0, None)
            self._c = _lib.CFieldBcs(*[(default if self.sides[k] is None else self.sides[k].c_struct(grid, k)) for k in self.SIDES])
        return self._c
