"""scptoolbox.jl_amd -- MI355X-native SCP inner loop behind the SCPToolbox.jl
solver contract (discretize! + solve_subproblem! under PTR).

The directory name contains a dot, so it cannot be imported with a plain
`import`; use `__graft_entry__.load_package()` (registers it as
`scptoolbox_jl_amd`).
"""
from . import _lib  # noqa: F401
from .models import REGISTRY, NativeModel  # noqa: F401
from .scp import FOH, IMPULSE, DLTV, SCPProblem, SCPScaling, SubproblemSolutionBatch, discretize_, propagate, continuous_time, LinearTrajectory, ImpulseTrajectory, device_guess, device_guess_failures  # noqa: F401
# (the package attribute `audit` is the function, as before; the module audit.py is imported by name: `from .audit import ...`)
from .audit import audit,audit_resident, AuditBatch, audit_intervals, audit_intervals_resident, IntervalAuditBatch, audit_dispersed, audit_dispersed_resident, DispersedAuditBatch, lqr_gains, lqr_gains_resident, GainBatch, audit_tracking, audit_tracking_resident, TrackingAuditBatch, audit_covariance, audit_covariance_resident, CovarianceAuditBatch, audit_montecarlo, audit_montecarlo_resident, MonteCarloAuditBatch  # noqa: F401
from .problem import TrajectoryProblem  # noqa: F401
from . import ptr as PTR  # noqa: F401
from . import dist  # noqa: F401
from . import homotopy  # noqa: F401
from .homotopy import Homotopy  # noqa: F401
from . import conic  # noqa: F401
from . import affine, subproblem, generic  # noqa: F401
from . import scvx as SCvx  # noqa: F401
from . import gusto as GuSTO  # noqa: F401
