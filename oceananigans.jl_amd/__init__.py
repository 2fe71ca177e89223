"""oceananigans.jl_amd -- MI355X-native NonhydrostaticModel time-stepping hot path of Oceananigans.jl.

Host-side mirror of the reference's operator surface (Architectures / Grids / Fields / Advection / Solvers /
TimeSteppers / Models.NonhydrostaticModels / DistributedComputations) over the C ABI of libocn_hip.so.
The directory name contains a dot, so import it through the root-level shim:

    import oceananigans_jl_amd as ocn
"""
from . import _lib
from ._lib import MATH_FAST, MATH_STRICT, OcnError
from .advection import WENO, UpwindBiased
from .architectures import CPU, GPU, on_architecture, sync_device, zeros
from .distributed import (Distributed, DistributedFFTBasedPoissonSolver, DistributedFourierTridiagonalPoissonSolver, Partition,
                          TorchDistributedFabric)
from .fields import CenterField, Field, XFaceField, YFaceField, ZFaceField, fill_halo_regions, mask_immersed_field
from .grids import Bounded, Center, Face, Flat, FullyConnected, LeftConnected, Periodic, RectilinearGrid, RightConnected
from .grids import (CenterImmersedCondition, GridFittedBottom, GridFittedBoundary, ImmersedBoundaryGrid, InterfaceImmersedCondition,
                    PartialCellBottom, immersed_cell, immersed_inactive_node, immersed_peripheral_node, inactive_node, peripheral_node,
                    static_column_depth)
from .models import (NonhydrostaticModel, QuasiAdamsBashforth2TimeStepper, RungeKutta3TimeStepper, ab2_step,
                     cache_previous_tendencies, calculate_pressure_correction, compute_auxiliaries, compute_diffusivities,
                     compute_tendencies, flush_tendencies, RK3Driver, ModelRK3Driver, implicit_step, add_vertically_implicit_explicit_fluxes,
                     pressure_correct_velocities, rk3_substep, set, solve_for_pressure, time_step, update_hydrostatic_pressure,
                     update_state, compute_boundary_functions, compute_boundary_tendency_contributions, add_forcing_programs)
from .output import (AdvectiveCFL, DiffusiveCFL, NaNChecker, TimeStepWizard, cell_advection_timescale, cell_diffusion_timescale, hasnan, set_from_checkpoint,
                     write_checkpoint)
from .physics import (HorizontalDivergenceFormulation, HorizontalFormulation, HorizontalScalarBiharmonicDiffusivity, ScalarBiharmonicDiffusivity,
                      ThreeDimensionalFormulation, VerticalFormulation)
from .physics import (ExponentialRiDependentTapering, FivePointHorizontalFilter, HyperbolicTangentRiDependentTapering,
                      PiecewiseLinearRiDependentTapering, RiBasedVerticalDiffusivity)
from .physics import CATKEEquation, CATKEMixingLength, CATKEVerticalDiffusivity
from .physics import (ConstantStabilityFunctions, StratifiedDisplacementScale, TKEDissipationEquations, TKEDissipationVerticalDiffusivity,
                      VariableStabilityFunctions)
from .physics import (AdvectiveFormulation, DiffusiveFormulation, FluxTapering, IsopycnalSkewSymmetricDiffusivity, IsopycnalTensor,
                      SmallSlopeIsopycnalTensor)
from .physics import (AnisotropicMinimumDissipation, ConvectiveAdjustmentVerticalDiffusivity, DynamicCoefficient, DynamicSmagorinsky, LillyCoefficient, Smagorinsky, SmagorinskyLilly, BetaPlane, BoundaryCondition, BuoyancyTracer, Centered, FieldBoundaryConditions, FluxBoundaryCondition, FPlane,
                      GradientBoundaryCondition, LinearEquationOfState, OpenBoundaryCondition, ScalarDiffusivity, SeawaterBuoyancy,
                      ValueBoundaryCondition, ExplicitTimeDiscretization, VerticallyImplicitTimeDiscretization)
from .stokes import StokesDrift, UniformStokesDrift
from .particles import (LagrangianParticles, advect_lagrangian_particles, step_lagrangian_particles,
                        update_lagrangian_particle_properties)
from .forcings import AdvectiveForcing, ContinuousForcing, Forcing, GaussianMask, LinearTarget, Relaxation
from . import boundary_functions, forcing_programs
from .forcing_programs import ForcingProgram, ProgramForcing
from .boundary_functions import BoundaryFunction, BoundaryProgram
from .operations import (AbstractOperation, Average, BinaryOperation, ComputedField, CumulativeIntegral, Derivative, Integral,
                         KernelFunctionOperation, UnaryOperation, abs, at, compute, cos, ddx, ddy, ddz, exp, log, lower, maximum, minimum, sin, sqrt,
                         tanh)
from .solvers import (BatchedTridiagonalSolver, FFTBasedPoissonSolver, FourierTridiagonalPoissonSolver, XDirection, YDirection, ZDirection,
                      nonhydrostatic_pressure_solver, solve, stretched_direction)


from .hydrostatic import (AdamsBashforth3Scheme, ExplicitFreeSurface, ForwardBackwardScheme, HydrostaticFreeSurfaceModel, ImplicitFreeSurface, SplitExplicitFreeSurface,  # noqa: E402
                          VectorInvariant, WENOVectorInvariant, EnergyConserving, EnstrophyConserving, VelocityStencil, DefaultStencil,
                          FunctionStencil, OnlySelfUpwinding, CrossAndSelfUpwinding)


def set_math_mode(mode):
    """MATH_STRICT: reference evaluation order (bit-reproducible vs the CPU oracle); MATH_FAST: FMA + fused division."""
    _lib.call("ocn_set_math_mode", int(mode))
