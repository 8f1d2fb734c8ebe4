"""assistedmanipulation_amd — MI355X-native MPPI trajectory engine.

A drop-in for the reference's mppi::Trajectory hot path (LuigiVan01/AssistedManipulation,
src/controller/mppi.{hpp,cpp}) with the FrankaRidgeback Pinocchio dynamics and the
AssistedManipulation cost evaluated by hand-written HIP kernels for gfx950.  The native
library (lib/libmppi_amd.so, C-ABI in include/mppi_amd.h) is loaded at import; there is no
CPU fallback.
"""
from . import abi
from ._lib import load as _load

_load()   # fail loudly at import if the engine library is missing

from .config import (Configuration, Smoothing, average_forecast_configuration, constant_forecast,  # noqa: E402
                     frankaridgeback_configuration, huddled_state, kalman_forecast_configuration,
                     locf_forecast_configuration, point_mass_configuration)
from .trajectory import (AssistedManipulation, Cost, Dynamics, EngineError, TrackPoint,  # noqa: E402
                         FrankaRidgebackDynamics, PointMassDynamics, Predicted, QuadraticCost, Trajectory,
                         comm_unique_id, shard_range)

from .obstacles import (CapsuleObstacle, HalfSpaceObstacle, ObstacleAvoidance, ObstacleCapsules, SphereObstacle,  # noqa: E402
                        MASK_ALL, MASK_SEGMENTS, mask_segment, obstacle_clearance, obstacle_from_c, obstacles_to_c,
                        segment_distance)
from .distance_field import DistanceField, field_clearance  # noqa: E402
from .held_object import HeldObject, MASK_HELD, held_object_clearance, mask_held_point, mask_held_segment  # noqa: E402
from .held_self import HeldSelf, held_self_clearance, held_self_unit_point, held_self_unit_segment  # noqa: E402
from .targets import TargetPath, TargetTracking, quaternion_rotation  # noqa: E402
from .safety import TrajectorySafetyFilter  # noqa: E402
from .csvlog import MPPILogger  # noqa: E402
from .dynamics import DynamicsForecast, EndEffectorState, PinocchioDynamicsObject, evaluate_cost  # noqa: E402

__all__ = [
    "MPPILogger", "DynamicsForecast", "EndEffectorState", "PinocchioDynamicsObject", "evaluate_cost",
    "abi", "Configuration", "Smoothing", "constant_forecast", "frankaridgeback_configuration",
    "huddled_state", "point_mass_configuration", "locf_forecast_configuration", "average_forecast_configuration",
    "kalman_forecast_configuration", "AssistedManipulation", "TrackPoint", "Cost", "Dynamics",
    "EngineError", "FrankaRidgebackDynamics", "PointMassDynamics", "QuadraticCost", "Trajectory",
    "comm_unique_id", "shard_range", "Predicted", "ObstacleAvoidance", "SphereObstacle", "HalfSpaceObstacle",
    "obstacle_clearance", "TrajectorySafetyFilter", "CapsuleObstacle", "ObstacleCapsules", "MASK_ALL", "MASK_SEGMENTS",
    "mask_segment", "obstacle_from_c", "obstacles_to_c", "segment_distance", "DistanceField", "field_clearance",
    "TargetPath", "TargetTracking", "quaternion_rotation", "HeldObject", "MASK_HELD", "mask_held_point", "mask_held_segment",
    "held_object_clearance", "HeldSelf", "held_self_unit_point", "held_self_unit_segment", "held_self_clearance",
]
