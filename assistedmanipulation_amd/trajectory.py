"""mppi::Trajectory and its plugin surface on the MI355X engine.

Mirrors src/controller/mppi.hpp of the reference: `Trajectory.create(configuration, dynamics,
cost)` returns None on a validation failure (the reference returns nullptr and prints to stderr,
mppi.cpp:17-69); `update(state, time)` runs one MPPI iteration on the device; `get(control,
time)` / `__call__(time)` interpolate the published optimal control; the accessors return the
quantities logger::MPPI records (logging/mppi.cpp:84-136).

The dynamics and cost are *descriptors* (POD parameter blocks) rather than virtual objects: the
kernels evaluate them on the device.  FrankaRidgebackDynamics / AssistedManipulation replace
FrankaRidgeback::PinocchioDynamics / FrankaRidgeback::AssistedManipulation;
PointMassDynamics / QuadraticCost are the bring-up plugins of SURVEY §8a a16.
"""
import ctypes as C
import sys

import numpy as np

from . import abi
from ._lib import load
from .obstacles import ObstacleAvoidance, ObstacleCapsules, obstacle_from_c, obstacles_to_c
from .targets import TargetPath, TargetTracking
from .config import Configuration
from .safety import TrajectorySafetyFilter


class EngineError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s: %s" % (abi.STATUS_NAMES.get(status, status), message))
        self.status = status


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---- plugin descriptors -------------------------------------------------------------------
class Dynamics:
    """mppi::Dynamics (mppi.hpp:30-85) as a device descriptor."""
    control_dof = None
    state_dof = None

    def descriptor(self):
        raise NotImplementedError

    def get_control_dof(self):
        return self.control_dof

    def get_state_dof(self):
        return self.state_dof


class Cost:
    """mppi::Cost (mppi.hpp:93-145) as a device descriptor."""
    control_dof = None
    state_dof = None

    def descriptor(self):
        raise NotImplementedError

    def get_control_dof(self):
        return self.control_dof

    def get_state_dof(self):
        return self.state_dof


class FrankaRidgebackDynamics(Dynamics):
    """FrankaRidgeback::PinocchioDynamics (pinocchio_dynamics.{hpp,cpp}).  `model` is a
    mppi_frankaridgeback_desc; by default the body table generated from robot.urdf.
    `link_positions`: what get_link_position answers in the rollouts (mppi_set_link_positions) -
    True the kinematic model (the links' body-frame translations of the last calculate(), a live
    self-collision term), False the reference's stub (zeros), None what MPPI_LINK_POSITIONS says
    (unset: the stub).
    `simulated_wrench`: the end-effector wrench the rollouts' dynamics feel
    (mppi_set_simulated_wrench) - "state" the wrench slots of the update's state at every step,
    "forecast" row k of the forecast the objective reads at step k, False none (the reference's
    stub), None what MPPI_SIMULATED_WRENCH says (unset: none)."""
    control_dof = abi.MPPI_FR_CONTROL
    state_dof = abi.MPPI_FR_STATE
    SIMULATED_WRENCH_MODES = {False: abi.MPPI_SIMULATED_WRENCH_OFF, "state": abi.MPPI_SIMULATED_WRENCH_STATE,
                              "forecast": abi.MPPI_SIMULATED_WRENCH_FORECAST}

    def __init__(self, model=None, link_positions=None, simulated_wrench=None):
        if simulated_wrench is not None and simulated_wrench not in self.SIMULATED_WRENCH_MODES:
            raise ValueError('simulated_wrench must be None, False, "state" or "forecast"')
        self.simulated_wrench = simulated_wrench
        if model is None:
            model = abi.mppi_frankaridgeback_desc()
            load().mppi_default_frankaridgeback(C.byref(model))
        self.model = model
        self.link_positions = None if link_positions is None else bool(link_positions)

    def descriptor(self):
        d = abi.mppi_dynamics_desc()
        d.kind = abi.MPPI_DYNAMICS_FRANKARIDGEBACK
        d.frankaridgeback = self.model
        return d


class PointMassDynamics(Dynamics):
    control_dof = 3
    state_dof = 6

    def __init__(self, mass=1.0):
        self.mass = mass

    def descriptor(self):
        d = abi.mppi_dynamics_desc()
        d.kind = abi.MPPI_DYNAMICS_POINT_MASS
        d.point_mass.mass = self.mass
        return d


class AssistedManipulation(Cost):
    """FrankaRidgeback::AssistedManipulation (objective/assisted_manipulation.{hpp,cpp}).
    `configuration` is a mppi_assisted_manipulation_desc; by default DEFAULT_CONFIGURATION."""
    control_dof = abi.MPPI_FR_CONTROL
    state_dof = abi.MPPI_FR_STATE

    def __init__(self, configuration=None):
        if configuration is None:
            configuration = abi.mppi_assisted_manipulation_desc()
            load().mppi_default_assisted_manipulation(C.byref(configuration))
        self.configuration = configuration

    def descriptor(self):
        c = abi.mppi_cost_desc()
        c.kind = abi.MPPI_COST_ASSISTED_MANIPULATION
        c.assisted_manipulation = self.configuration
        return c


class TrackPoint(Cost):
    """FrankaRidgeback::TrackPoint (objective/track_point.{hpp,cpp}).
    `configuration` is a mppi_track_point_desc; by default DEFAULT_CONFIGURATION; `point`
    overrides the tracked point."""
    control_dof = abi.MPPI_FR_CONTROL
    state_dof = abi.MPPI_FR_STATE

    def __init__(self, configuration=None, point=None):
        if configuration is None:
            configuration = abi.mppi_track_point_desc()
            load().mppi_default_track_point(C.byref(configuration))
        if point is not None:
            for i in range(3):
                configuration.point[i] = float(point[i])
        self.configuration = configuration

    def descriptor(self):
        c = abi.mppi_cost_desc()
        c.kind = abi.MPPI_COST_TRACK_POINT
        c.track_point = self.configuration
        return c


class QuadraticCost(Cost):
    control_dof = 3
    state_dof = 6

    def __init__(self, target=(1.0, 1.0, 1.0), q=(1.0, 1.0, 1.0), r=(0.01, 0.01, 0.01)):
        self.target, self.q, self.r = target, q, r

    def descriptor(self):
        c = abi.mppi_cost_desc()
        c.kind = abi.MPPI_COST_QUADRATIC
        for i in range(3):
            c.quadratic.target[i] = self.target[i]
            c.quadratic.q[i] = self.q[i]
            c.quadratic.r[i] = self.r[i]
        return c


def shard_range(rollout_count, world, rank):
    b, e = C.c_int64(), C.c_int64()
    st = load().mppi_shard_range(rollout_count, world, rank, C.byref(b), C.byref(e))
    if st != abi.MPPI_OK:
        raise EngineError(st, "invalid shard (%d, %d, %d)" % (rollout_count, world, rank))
    return b.value, e.value


def comm_unique_id():
    buf = C.create_string_buffer(128)
    st = load().mppi_comm_unique_id(buf)
    if st != abi.MPPI_OK:
        raise EngineError(st, "ncclGetUniqueId failed")
    return buf.raw


class Predicted:
    """Predicted trajectories (mppi_predicted_optimal / mppi_predicted_rollouts): `raw` is the
    (..., H, MPPI_PRED_N) array, the rest are views of it.  Row k is the state x_k at which step k's
    cost is evaluated (row 0 the update's state) at `time[k]` = t0 + k dt; the positions are forward
    kinematics at q_k itself.  `energy` is NaN unless the rollouts integrate the tank; from a
    rollout's first non-finite state on, its rows are NaN.  `rollouts`: the indices asked for (None
    for the optimal rollout)."""

    def __init__(self, raw, t0, dt, rollouts=None):
        H = raw.shape[-2]
        self.raw = raw
        self.rollouts = rollouts
        self.time = t0 + np.arange(H) * dt
        self.position = raw[..., abi.MPPI_PRED_Q:abi.MPPI_PRED_Q + 12]
        self.velocity = raw[..., abi.MPPI_PRED_QD:abi.MPPI_PRED_QD + 12]
        self.energy = raw[..., abi.MPPI_PRED_ENERGY]
        self.end_effector = raw[..., abi.MPPI_PRED_EE:abi.MPPI_PRED_EE + 3]
        self.arm_mount = raw[..., abi.MPPI_PRED_ARM_MOUNT:abi.MPPI_PRED_ARM_MOUNT + 3]
        self.links = raw[..., abi.MPPI_PRED_LINKS:abi.MPPI_PRED_N].reshape(raw.shape[:-1] + (abi.MPPI_LINK_N, 3))


class CUpdateEntry(tuple):
    """(fn, handle, state pointer) of Trajectory.c_update_entry, holding the Trajectory alive."""

    def __new__(cls, items, trajectory):
        t = super().__new__(cls, items)
        t.trajectory = trajectory
        return t


class Trajectory:
    """mppi::Trajectory (mppi.hpp:267-658) on one MI355X device."""

    def __init__(self, handle, configuration, dynamics, cost):
        self._L = load()
        self._h = handle
        self.configuration = configuration
        self.dynamics = dynamics
        self.cost = cost
        self._field_values = None
        R, H, Cc, X = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._L.mppi_dims(self._h, C.byref(R), C.byref(H), C.byref(Cc), C.byref(X)))
        self.R, self.H, self.C, self.X = R.value, H.value, Cc.value, X.value
        self._rolled_out_state = np.asarray(configuration.initial_state, dtype=np.float64).copy()
        self._rolled_out_state[:] = 0.0   # m_rollout_state.setZero() (mppi.cpp:121)
        self._state_buf = np.zeros(self.X, dtype=np.float64)
        self._state_ptr = _p(self._state_buf)

    @staticmethod
    def create(configuration: Configuration, dynamics: Dynamics, cost: Cost, device=0, filter=None):
        """Trajectory::create — None (and a message on stderr) on invalid input.  `filter`: a
        TrajectorySafetyFilter applied to every update's plan, or None."""
        L = load()
        cfg, keep = configuration.to_c()
        dd, cd = dynamics.descriptor(), cost.descriptor()
        h = C.c_void_p()
        st = L.mppi_create(C.byref(cfg), C.byref(dd), C.byref(cd), int(device), C.byref(h))
        del keep
        if st != abi.MPPI_OK:
            print(L.mppi_last_error(None).decode(), file=sys.stderr)
            return None
        t = Trajectory(h, configuration, dynamics, cost)
        lp = getattr(dynamics, "link_positions", None)
        if lp is not None:   # FrankaRidgebackDynamics(link_positions=...)
            t.set_link_positions(abi.MPPI_LINK_POSITIONS_KINEMATIC if lp else abi.MPPI_LINK_POSITIONS_ZERO)
        sw = getattr(dynamics, "simulated_wrench", None)
        if sw is not None:   # FrankaRidgebackDynamics(simulated_wrench=...)
            t.set_simulated_wrench(FrankaRidgebackDynamics.SIMULATED_WRENCH_MODES[sw])
        if filter is not None:
            try:
                t.set_safety_filter(filter)
            except EngineError as e:   # the reference's create prints and returns nullptr
                print(str(e), file=sys.stderr)
                t.close()
                return None
        return t

    # -- lifecycle --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.mppi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != abi.MPPI_OK:
            raise EngineError(st, self._L.mppi_last_error(self._h).decode())

    # -- multi-GPU ---------------------------------------------------------------------------
    def comm_init(self, world, rank, unique_id):
        self._check(self._L.mppi_comm_init(self._h, world, rank, unique_id))

    def comm_info(self):
        """The engine communicator as RCCL reports it: {"nranks", "rank"} (0 / -1 without one), and
        the handle's HIP device and PCI bus id (mppi_comm_info)."""
        n, r, d = C.c_int(), C.c_int(), C.c_int()
        bus = C.create_string_buffer(64)
        self._check(self._L.mppi_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d), bus, 64))
        return {"nranks": n.value, "rank": r.value, "device": d.value, "pci_bus_id": bus.value.decode()}

    def set_shard(self, world, rank):
        self._check(self._L.mppi_set_shard(self._h, world, rank))

    # -- parity hooks ------------------------------------------------------------------------
    def set_link_positions(self, mode):
        """mppi_set_link_positions: abi.MPPI_LINK_POSITIONS_*; FrankaRidgeback handles, before the
        first update."""
        self._check(self._L.mppi_set_link_positions(self._h, int(mode)))

    @property
    def link_positions(self):
        """Whether the rollouts use the kinematic link-position model (read-only; False for a
        handle without links)."""
        m = C.c_int(0)
        st = self._L.mppi_get_link_positions(self._h, C.byref(m))
        if st == abi.MPPI_ERR_UNSUPPORTED:
            return False
        self._check(st)
        return m.value == abi.MPPI_LINK_POSITIONS_KINEMATIC

    def set_simulated_wrench(self, mode):
        """mppi_set_simulated_wrench: abi.MPPI_SIMULATED_WRENCH_OFF / _STATE / _FORECAST;
        FrankaRidgeback handles, before the first update."""
        self._check(self._L.mppi_set_simulated_wrench(self._h, int(mode)))

    @property
    def simulated_wrench(self):
        """The rollouts' simulated-wrench mode (abi.MPPI_SIMULATED_WRENCH_*, read-only;
        MPPI_SIMULATED_WRENCH_OFF for a handle without the FrankaRidgeback dynamics)."""
        m = C.c_int(0)
        st = self._L.mppi_get_simulated_wrench(self._h, C.byref(m))
        if st == abi.MPPI_ERR_UNSUPPORTED:
            return abi.MPPI_SIMULATED_WRENCH_OFF
        self._check(st)
        return m.value

    def set_safety_filter(self, filter):
        """mppi_set_safety_filter: a TrajectorySafetyFilter, or None to turn it off; between any two
        updates.  FrankaRidgeback handles only.  With a filter set every update publishes the
        filtered plan (and does not run as a hipGraph)."""
        if filter is None:
            self._check(self._L.mppi_set_safety_filter(self._h, None))
            return
        c = filter.to_c()
        self._check(self._L.mppi_set_safety_filter(self._h, C.byref(c)))

    @property
    def safety_filter(self):
        """The TrajectorySafetyFilter the handle runs with, or None."""
        on, c = C.c_int(0), abi.mppi_safety_filter_desc()
        st = self._L.mppi_get_safety_filter(self._h, C.byref(on), C.byref(c))
        if st == abi.MPPI_ERR_UNSUPPORTED:
            return None
        self._check(st)
        return TrajectorySafetyFilter.from_c(c) if on.value else None

    def unfiltered_control(self):
        """mppi_unfiltered_control: the last update's plan as optimise() left it, before the safety
        filter, (H, C) like get_optimal_rollout (which it equals without a filter)."""
        return self._vec(self._L.mppi_unfiltered_control, self.C * self.H).reshape(self.H, self.C)

    def safety_filter_stats(self):
        """{"changed_steps": steps of the last update's plan the filter changed, "kernel_ms": the
        filter kernel's time (0 unless set_timing(1) or (2))}."""
        n, ms = C.c_int64(0), C.c_float(0.0)
        self._check(self._L.mppi_safety_filter_stats(self._h, C.byref(n), C.byref(ms)))
        return {"changed_steps": n.value, "kernel_ms": ms.value}

    def set_obstacle_avoidance(self, config=None):
        """mppi_set_obstacle_avoidance: sphere and half-space obstacles in the rollouts' objective,
        with `config` (an ObstacleAvoidance; None: the defaults).  FrankaRidgeback handles in the
        kinematic link-position model, before the first update; fixed for the handle's life."""
        c = (config or ObstacleAvoidance()).to_c()
        self._check(self._L.mppi_set_obstacle_avoidance(self._h, C.byref(c)))

    @property
    def obstacle_avoidance(self):
        """The ObstacleAvoidance configuration the handle runs with, or None when it is off."""
        on, c = C.c_int(0), abi.mppi_obstacle_config()
        self._check(self._L.mppi_get_obstacle_avoidance(self._h, C.byref(on), C.byref(c)))
        return ObstacleAvoidance.from_c(c) if on.value else None

    def set_obstacle_capsules(self, capsules=None):
        """mppi_set_obstacle_capsules: the robot's eight segments (the links between consecutive robot
        points) and capsule obstacles in the obstacle term, with `capsules` (an ObstacleCapsules; None:
        the defaults).  After set_obstacle_avoidance and before the first update; it cannot be undone."""
        c = (capsules or ObstacleCapsules()).to_c()
        self._check(self._L.mppi_set_obstacle_capsules(self._h, C.byref(c)))

    @property
    def obstacle_capsules(self):
        """The ObstacleCapsules configuration the handle runs with, or None without capsules."""
        on, c = C.c_int(0), abi.mppi_capsule_config()
        self._check(self._L.mppi_get_obstacle_capsules(self._h, C.byref(on), C.byref(c)))
        return ObstacleCapsules.from_c(c) if on.value else None

    def set_distance_field_avoidance(self):
        """mppi_set_distance_field_avoidance: a signed-distance grid of the sensed environment in the
        obstacle term, behind the capsule term.  After set_obstacle_capsules and before the first
        update; it cannot be undone."""
        self._check(self._L.mppi_set_distance_field_avoidance(self._h))

    @property
    def distance_field_avoidance(self):
        on = C.c_int(0)
        self._check(self._L.mppi_get_distance_field_avoidance(self._h, C.byref(on)))
        return bool(on.value)

    def set_distance_field(self, field):
        """mppi_set_distance_field: replace the field (a DistanceField; None: no field).  Between any
        two updates; every rank of a sharded run sets the same one.  The values are copied."""
        if field is None:
            self._check(self._L.mppi_set_distance_field(self._h, None, None))
        else:
            f = field.to_c()
            self._check(self._L.mppi_set_distance_field(self._h, C.byref(f), field.values_ptr()))
        self._field_values = None if field is None else field.values

    @property
    def distance_field(self):
        """The current DistanceField (the descriptor from mppi_get_distance_field, with the values
        this object was given), or None with no field."""
        f, on = abi.mppi_distance_field(), C.c_int(0)
        self._check(self._L.mppi_get_distance_field(self._h, C.byref(f), C.byref(on)))
        if not on.value:
            return None
        from .distance_field import DistanceField
        return DistanceField(self._field_values, list(f.origin), f.voxel, f.mask, f.segment_samples)

    def get_optimal_field_cost(self):
        """mppi_optimal_field_cost: the field term of the last update's filter() row summed over its
        steps, undiscounted (get_optimal_obstacle_cost holds it too, beside the capsule term)."""
        v = C.c_double(0.0)
        self._check(self._L.mppi_optimal_field_cost(self._h, C.byref(v)))
        return v.value

    def set_held_object_avoidance(self):
        """mppi_set_held_object_avoidance: a held object (spheres fixed in the grasp frame) in the
        obstacle term, behind the field term.  After set_distance_field_avoidance and before the first
        update; it cannot be undone."""
        self._check(self._L.mppi_set_held_object_avoidance(self._h))

    @property
    def held_object_avoidance(self):
        on = C.c_int(0)
        self._check(self._L.mppi_get_held_object_avoidance(self._h, C.byref(on)))
        return bool(on.value)

    def set_held_object(self, obj):
        """mppi_set_held_object: replace the object (a HeldObject; None: it was put down).  Between
        any two updates; every rank of a sharded run sets the same one."""
        if obj is None:
            self._check(self._L.mppi_set_held_object(self._h, None))
        else:
            o = obj.to_c()
            self._check(self._L.mppi_set_held_object(self._h, C.byref(o)))

    @property
    def held_object(self):
        """The current HeldObject (mppi_get_held_object), or None with nothing held."""
        o, on = abi.mppi_held_object(), C.c_int(0)
        self._check(self._L.mppi_get_held_object(self._h, C.byref(o), C.byref(on)))
        if not on.value:
            return None
        from .held_object import HeldObject
        return HeldObject.from_c(o)

    def get_optimal_held_cost(self):
        """mppi_optimal_held_cost: the held term of the last update's filter() row summed over its
        steps, undiscounted (get_optimal_obstacle_cost holds it too, beside the capsule and field terms)."""
        v = C.c_double(0.0)
        self._check(self._L.mppi_optimal_held_cost(self._h, C.byref(v)))
        return v.value

    def set_held_self_avoidance(self):
        """mppi_set_held_self_avoidance: the held object against the robot's own segments in the
        obstacle term, behind the held term.  After set_held_object_avoidance and before the first
        update; it cannot be undone."""
        self._check(self._L.mppi_set_held_self_avoidance(self._h))

    @property
    def held_self_avoidance(self):
        on = C.c_int(0)
        self._check(self._L.mppi_get_held_self_avoidance(self._h, C.byref(on)))
        return bool(on.value)

    def set_held_self(self, cfg):
        """mppi_set_held_self: replace the configuration (a HeldSelf; None: none).  Between any two
        updates; every rank of a sharded run sets the same one."""
        if cfg is None:
            self._check(self._L.mppi_set_held_self(self._h, None))
        else:
            c = cfg.to_c()
            self._check(self._L.mppi_set_held_self(self._h, C.byref(c)))

    @property
    def held_self(self):
        """The current HeldSelf (mppi_get_held_self), or None with no configuration."""
        c, on = abi.mppi_held_self(), C.c_int(0)
        self._check(self._L.mppi_get_held_self(self._h, C.byref(c), C.byref(on)))
        if not on.value:
            return None
        from .held_self import HeldSelf
        return HeldSelf.from_c(c)

    def get_optimal_held_self_cost(self):
        """mppi_optimal_held_self_cost: the held-self term of the last update's filter() row summed over
        its steps, undiscounted (get_optimal_obstacle_cost holds it too, beside the other three parts)."""
        v = C.c_double(0.0)
        self._check(self._L.mppi_optimal_held_self_cost(self._h, C.byref(v)))
        return v.value

    def predicted_held_optimal(self):
        """mppi_predicted_held_optimal: where the held points go under the published plan, (H, 4, 3)
        world positions at q_k itself (not lagged); the rows of points the object does not have are NaN."""
        raw = np.zeros((self.H, abi.MPPI_HELD_POINTS, 3))
        self._check(self._L.mppi_predicted_held_optimal(self._h, _p(raw)))
        return raw

    def predicted_held_rollouts(self, indices):
        """mppi_predicted_held_rollouts: the same for rollouts of the last update by global index,
        (n, H, 4, 3) in the order of `indices`."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        raw = np.zeros((idx.size, self.H, abi.MPPI_HELD_POINTS, 3))
        self._check(self._L.mppi_predicted_held_rollouts(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, _p(raw)))
        return raw

    def set_obstacles(self, obstacles, time):
        """mppi_set_obstacles: replace the whole set (SphereObstacle / HalfSpaceObstacle, at most 16;
        an empty list clears it), given at reference time `time`.  Between any two updates; every
        rank of a sharded run sets the same one."""
        arr, n = obstacles_to_c(obstacles)
        self._check(self._L.mppi_set_obstacles(self._h, arr, n, float(time)))

    def obstacles(self):
        """(the current set as a list, its reference time) (mppi_get_obstacles)."""
        arr = (abi.mppi_obstacle * abi.MPPI_MAX_OBSTACLES)()
        n, t = C.c_int32(0), C.c_double(0.0)
        self._check(self._L.mppi_get_obstacles(self._h, arr, C.byref(n), C.byref(t)))
        return [obstacle_from_c(arr[i]) for i in range(n.value)], t.value

    def get_optimal_obstacle_cost(self):
        """mppi_optimal_obstacle_cost: the obstacle term of the last update's filter() row summed over
        its steps, undiscounted, next to get_optimal_terms' seven totals."""
        v = C.c_double(0.0)
        self._check(self._L.mppi_optimal_obstacle_cost(self._h, C.byref(v)))
        return v.value

    def set_target_tracking(self, config=None):
        """mppi_set_target_tracking: TrackPoint follows a timed pose path (set_target_path) instead of
        its fixed point, with `config` (a TargetTracking; None: the defaults, position only).
        FrankaRidgeback handles with the TrackPoint objective, before the first update; orientation
        tracking needs the kinematic link-position model.  It cannot be undone."""
        c = (config or TargetTracking()).to_c()
        self._check(self._L.mppi_set_target_tracking(self._h, C.byref(c)))

    @property
    def target_tracking(self):
        """The TargetTracking in force, or None when tracking is off (mppi_get_target_tracking)."""
        on, c = C.c_int(0), abi.mppi_target_tracking_config()
        self._check(self._L.mppi_get_target_tracking(self._h, C.byref(on), C.byref(c)))
        return TargetTracking.from_c(c) if on.value else None

    def set_target_path(self, path):
        """mppi_set_target_path: replace the path (a TargetPath, or a raw abi.mppi_target_path; None
        clears it, and the target is the objective's point again).  Between any two updates; every
        rank of a sharded run sets the same one."""
        if path is None:
            self._check(self._L.mppi_set_target_path(self._h, None))
            return
        c = path if isinstance(path, abi.mppi_target_path) else path.to_c()
        self._check(self._L.mppi_set_target_path(self._h, C.byref(c)))

    def target_path(self):
        """The current path as the engine stored it (quaternions normalised and sign-fixed), or None
        (mppi_get_target_path)."""
        c, present = abi.mppi_target_path(), C.c_int(0)
        self._check(self._L.mppi_get_target_path(self._h, C.byref(c), C.byref(present)))
        return TargetPath.from_c(c) if present.value else None

    def get_optimal_target_cost(self):
        """mppi_optimal_target_cost: (position total, orientation total) of the last update's filter()
        row over its steps, undiscounted."""
        o = np.zeros(2)
        self._check(self._L.mppi_optimal_target_cost(self._h, _p(o)))
        return float(o[0]), float(o[1])

    def set_noise_source(self, source, seed=0x5EED):
        self._check(self._L.mppi_set_noise_source(self._h, int(source), int(seed)))

    def inject_noise(self, eps):
        e = np.ascontiguousarray(eps, dtype=np.float64).reshape(-1)
        self._check(self._L.mppi_inject_noise(self._h, _p(e), e.size // self.C))

    def noise_draws(self, time):
        n = C.c_int64()
        self._check(self._L.mppi_noise_draws(self._h, float(time), C.byref(n)))
        return n.value

    def set_index_semantics(self, semantics):
        self._check(self._L.mppi_set_index_semantics(self._h, int(semantics)))

    def set_forecast(self, wrench_Hx6):
        if wrench_Hx6 is None:
            self._check(self._L.mppi_set_forecast(self._h, None))
            return
        t = np.ascontiguousarray(wrench_Hx6, dtype=np.float64)
        assert t.shape == (self.H, 6), t.shape
        self._check(self._L.mppi_set_forecast(self._h, _p(t)))

    # -- device wrench forecast -------------------------------------------
    def attach_forecast(self, configuration):
        """Forecast::create bound to the engine (forecast.cpp:6-39): every update then samples
        forecast(t0 + k dt) on the device.  None detaches (back to set_forecast tables)."""
        self._check(self._L.mppi_forecast_attach(self._h, None if configuration is None else C.byref(configuration)))

    def observe_wrench(self, wrench, time):
        """DynamicsForecast::observe_wrench (dynamics.hpp:221-224)."""
        w = np.ascontiguousarray(wrench, dtype=np.float64)
        assert w.size == 6
        self._check(self._L.mppi_forecast_observe(self._h, _p(w), float(time)))

    def observe_time(self, time):
        """DynamicsForecast::observe_time (dynamics.hpp:231-234)."""
        self._check(self._L.mppi_forecast_observe_time(self._h, float(time)))

    def forecast(self, time):
        """Forecast::forecast(time): the wrench the rollout's cost sees at `time`."""
        out = np.zeros(6)
        self._check(self._L.mppi_forecast_get(self._h, float(time), _p(out)))
        return out

    def forecast_table(self, t0, dt, steps):
        """[steps x 6]: forecast(t0 + k dt) of the attached device forecast (mppi_forecast_table)."""
        out = np.zeros((int(steps), 6))
        self._check(self._L.mppi_forecast_table(self._h, float(t0), float(dt), int(steps), _p(out)))
        return out

    def step_constants(self):
        """Parity hook: [H x 8] per-step trajectory-cost constants of the last update."""
        out = np.zeros((self.H, 8))
        self._check(self._L.mppi_step_constants(self._h, _p(out)))
        return out

    # -- the hot path ------------------------------------------------------------------------
    def update(self, state, time):
        """Trajectory::update (mppi.cpp:154-187)."""
        buf = self._state_buf   # one contiguous buffer and its pointer, built once: the update
        if type(state) is np.ndarray and state.shape == buf.shape:   # path is latency-bound: the usual
            buf[...] = state                                         # case in one copy (~0.7 us, not ~2.6)
        else:
            if np.size(state) != self.X:
                raise ValueError("state must have %d entries, got %d" % (self.X, np.size(state)))
            np.copyto(buf, np.reshape(state, -1))
        st = self._L.mppi_update(self._h, self._state_ptr, float(time))
        if st != abi.MPPI_OK:
            self._check(st)
        self._rolled_out_state = buf   # copied when queried (get_rolled_out_state)

    def c_update_entry(self, state):
        """The C-ABI update entry for a caller that drives its own loop, as a C++ caller of
        include/mppi_amd.hpp does: returns (fn, handle, state pointer), with `state` copied into
        the handle's state buffer once; fn(handle, pointer, time) is mppi_update (mppi.cpp:154-187)
        and returns an mppi_status (abi.MPPI_OK = 0).  Change the state by writing the buffer
        (self.state_buffer) in place.  The update count and time live in the engine
        (get_update_count / get_update_last read them), so updates made through it count.
        Lifetime: the handle and the pointer are this Trajectory's; the returned entry holds a
        reference to it (entry.trajectory), so keep the entry - or the Trajectory - alive while
        calling fn (after close() or garbage collection the handle is freed)."""
        buf = self._state_buf
        if np.size(state) != self.X:
            raise ValueError("state must have %d entries, got %d" % (self.X, np.size(state)))
        np.copyto(buf, np.reshape(np.asarray(state, dtype=np.float64), -1))
        self._rolled_out_state = buf
        return CUpdateEntry((self._L.mppi_update, self._h, self._state_ptr), self)

    @property
    def state_buffer(self):
        """The state buffer c_update_entry's pointer points at."""
        return self._state_buf

    def set_graph(self, enable):
        """The hipGraph path of update() (mppi_set_graph): the steady-state update as one graph launch."""
        self._check(self._L.mppi_set_graph(self._h, int(bool(enable))))

    def graph_updates(self):
        """How many updates ran as the captured graph (mppi_graph_updates)."""
        n = C.c_int64()
        self._check(self._L.mppi_graph_updates(self._h, C.byref(n)))
        return n.value

    def synchronize(self):
        """Wait for all device work of this handle (including the overlapped filter())."""
        self._check(self._L.mppi_synchronize(self._h))

    def update_phase1(self, state, time):
        s = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        if s.size != self.X:
            raise ValueError("state must have %d entries, got %d" % (self.X, s.size))
        self._check(self._L.mppi_update_phase1(self._h, _p(s), float(time)))
        self._rolled_out_state = s.copy()

    def update_phase2(self):
        self._check(self._L.mppi_update_phase2(self._h))

    def update_phase3(self, time):
        self._check(self._L.mppi_update_phase3(self._h))

    def device_costs_ptr(self):
        return self._L.mppi_device_costs(self._h)

    def device_gradient_ptr(self):
        return self._L.mppi_device_gradient(self._h)

    # -- queries -----------------------------------------------------------------------------
    def get(self, time, control=None):
        out = np.zeros(self.C) if control is None else control
        self._check(self._L.mppi_get(self._h, float(time), _p(out)))
        return out

    def __call__(self, time):
        return self.get(time)

    def get_state_dof(self):
        return self.X

    def get_control_dof(self):
        return self.C

    def get_time_step(self):
        return self.configuration.time_step

    def get_step_count(self):
        return self.H

    def get_update_duration(self):
        d = C.c_double()
        self._check(self._L.mppi_update_duration(self._h, C.byref(d)))
        return d.value

    def get_update_last(self):
        """Trajectory::get_update_last: the engine's own (every update entry counts)."""
        d = C.c_double()
        self._check(self._L.mppi_update_last(self._h, C.byref(d)))
        return d.value

    def get_update_count(self):
        """Trajectory::get_update_count: the engine's count of successful updates."""
        return self.update_info()["update_count"]

    def device_costs_count(self):
        """Doubles of device_costs_ptr() a phase-split caller all-reduces (R + 1)."""
        return int(self._L.mppi_device_costs_count(self._h))

    def get_rollout_count(self):
        return self.R

    def get_rolled_out_state(self):
        return self._rolled_out_state.copy()

    def _vec(self, fn, n):
        out = np.zeros(n)
        self._check(fn(self._h, _p(out)))
        return out

    def get_weights(self):
        return self._vec(self._L.mppi_weights, self.R)

    def get_gradient(self):
        """C x H (Eigen column-major) returned as an (H, C) array: row k = column k."""
        return self._vec(self._L.mppi_gradient, self.C * self.H).reshape(self.H, self.C)

    def costs(self):
        return self._vec(self._L.mppi_costs, self.R)

    def noise(self):
        return self._vec(self._L.mppi_noise, self.R * self.C * self.H).reshape(self.R, self.H, self.C)

    def get_rollouts(self):
        """[(noise (H, C), cost)] per rollout (mppi.hpp:422-424)."""
        n, c = self.noise(), self.costs()
        return [(n[r], c[r]) for r in range(self.R)]

    def get_optimal_rollout(self):
        return self._vec(self._L.mppi_optimal_control, self.C * self.H).reshape(self.H, self.C)

    trajectory = get_optimal_rollout

    def get_optimal_total_cost(self):
        d = C.c_double()
        self._check(self._L.mppi_optimal_cost(self._h, C.byref(d)))
        return d.value

    def get_optimal_terms(self):
        """The optimal rollout's seven AssistedManipulation term totals (joint limit, self collision,
        workspace, energy tank, joint velocity, trajectory, manipulability): the accumulators
        BaseTest / logger::AssistedManipulation read after filter() (mppi_optimal_terms)."""
        return self._vec(self._L.mppi_optimal_terms, 7)

    # -- predicted trajectories -------------------------------------------------------------
    def predicted_optimal(self):
        """Where the robot goes under the published plan (mppi_predicted_optimal): a Predicted of H
        rows, row k the state x_k of the optimal rollout and the positions at q_k."""
        raw = np.zeros((self.H, abi.MPPI_PRED_N))
        self._check(self._L.mppi_predicted_optimal(self._h, _p(raw)))
        return Predicted(raw, self.get_update_last(), self.get_time_step())

    def predicted_rollouts(self, indices):
        """The same for rollouts of the last update by global index (mppi_predicted_rollouts): a
        Predicted whose arrays lead with the rollout, in the order of `indices`."""
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        raw = np.zeros((idx.size, self.H, abi.MPPI_PRED_N))
        self._check(self._L.mppi_predicted_rollouts(self._h, idx.ctypes.data_as(C.POINTER(C.c_int64)), idx.size, _p(raw)))
        return Predicted(raw, self.get_update_last(), self.get_time_step(), idx)

    def predicted_best(self, n):
        """predicted_rollouts of the n rollouts with the lowest costs, in cost order: NaN costs last,
        equal costs by index (the engine's stable order of the costs)."""
        c = self.costs()
        order = np.argsort(np.where(np.isnan(c), np.inf, c), kind="stable")
        return self.predicted_rollouts(order[:max(0, min(int(n), self.R))])

    def argmin(self):
        i = C.c_int64()
        self._check(self._L.mppi_argmin(self._h, C.byref(i)))
        return i.value

    def update_info(self):
        """What the last update's rollout launch did (mppi_update_info): dict of the engine's own
        choices (cooperative kernel, folded filter(), objective in the launch, tail draws,
        sampling mode 0/1/2, rows rolled out, the step at which the fifth wave's rows moved off
        the doubled SIMD or -1, the in-launch waits that gave up in the last update - which then
        failed - and summed since create; finish_path: the kernel that finished the update,
        abi.MPPI_FINISH_*, -1 from the fused point-mass launch or a library without the slot)."""
        keys = ("cooperative", "folded_filter", "objective_in_launch", "tail_draws", "sampling", "rows", "handover",
                "wait_timeouts", "wait_timeouts_total", "fused_update", "graph_updates", "graph_failures",
                "update_count", "stage_work", "finish_path")
        out = np.zeros(abi.MPPI_UPDATE_INFO_N, dtype=np.int64)
        out[14] = -1
        # a library from before the finish_path slot takes one slot fewer, one from before stage_work two
        for n in (out.size, out.size - 1, out.size - 2):
            st = self._L.mppi_update_info(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), n)
            if st != abi.MPPI_ERR_INVALID:
                break
        self._check(st)
        return {k: int(v) for k, v in zip(keys, out)}

    def debug_inject(self, fault, updates=1):
        """Fault injection for the failure-detection tests (mppi_debug_inject): the next `updates`
        rollout launches carry fault bits `fault` (abi.MPPI_DEBUG_*)."""
        self._check(self._L.mppi_debug_inject(self._h, int(fault), int(updates)))

    def debug_folded_cost(self):
        """The previous update's filter() cost as the last launch folded it (mppi_debug_folded_cost;
        tests only: no pending filter() is run or waited for)."""
        v = C.c_double()
        self._check(self._L.mppi_debug_folded_cost(self._h, C.byref(v)))
        return v.value

    def smoothing_windows(self):
        """(uu, tt, start_idx) of the per-dimension SG windows (SavitzkyGolayFilter::get_windows)."""
        w = self.configuration.smoothing.window
        W = self.H + 2 * w + 1
        uu, tt = np.zeros((self.C, W)), np.zeros((self.C, W))
        st = np.zeros(self.C, dtype=np.int64)
        self._check(self._L.mppi_smoothing_windows(self._h, _p(uu), _p(tt),
                                                   st.ctypes.data_as(C.POINTER(C.c_int64))))
        return uu, tt, st

    def set_timing(self, level):
        """HIP-event timing of the update path: 0 none (default), 1 the rollout kernel alone,
        2 every phase (mppi_set_timing)."""
        self._check(self._L.mppi_set_timing(self._h, int(level)))

    def rollout_kernel_times(self):
        """The rollout launch's HIP-event times (ms) of the updates run at timing level 1 since the
        last call, oldest first (mppi_rollout_kernel_times)."""
        out = (C.c_float * 64)()
        n = C.c_int(0)
        self._check(self._L.mppi_rollout_kernel_times(self._h, out, 64, C.byref(n)))
        return list(out[:n.value])

    def kernel_times(self, wait=True, detail=False):
        """[sample, rollout, weight-reduce, optimal rollout, whole update] in ms (HIP events).
        wait=False does not wait for the overlapped optimal rollout ([3] may be an earlier one's).
        detail=True appends [5], the rollout (dynamics) kernel alone ([1] also spans the cost kernel),
        [6], the weights + gradient launch alone ([2] also spans the finish kernel; timing level
        2), and [7], the cost all-reduce ahead of it (RCCL-sharded; 0 otherwise); it implies
        wait=False."""
        if detail:
            out = (C.c_float * 8)()
            self._check(self._L.mppi_kernel_times_detail(self._h, out, 8))
            return list(out)
        out = (C.c_float * 5)()
        fn = self._L.mppi_kernel_times if wait else self._L.mppi_kernel_times_nowait
        self._check(fn(self._h, out))
        return list(out)
