"""FrankaRidgeback::PinocchioDynamics as a device object, and DynamicsForecast on top of it.

The reference's plugins are objects with their own state, used outside mppi::Trajectory too:
PinocchioDynamics has set_state / step / get_state / get_end_effector_state
(frankaridgeback/pinocchio_dynamics.{hpp,cpp}, the mppi::Dynamics surface of mppi.hpp:47-84), and
the Actor's DynamicsForecast rolls its own copy forward with zero control every controller period
(frankaridgeback/dynamics.cpp:104-138, actor.cpp:176-177).  Here the object's state lives in HBM
and every method is a device kernel (fr_object.hip, through mppi_dynamics_* of the C-ABI); the
host keeps only the bookkeeping the reference keeps on the caller's side (DynamicsForecast's
trajectories and its time parameterisation, dynamics.hpp:243-345).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi
from ._lib import load


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@dataclass
class EndEffectorState:
    """EndEffectorState (dynamics.hpp:95-117) of a calculate()."""
    position: np.ndarray
    orientation: np.ndarray          # quaternion, Eigen coefficient order (x, y, z, w)
    rotation: np.ndarray             # the same orientation, 3 x 3
    linear_velocity: np.ndarray
    angular_velocity: np.ndarray
    linear_acceleration: np.ndarray
    angular_acceleration: np.ndarray
    jacobian: np.ndarray             # 6 x 12, WORLD

    @staticmethod
    def from_row(r):
        r = np.asarray(r, dtype=np.float64)
        return EndEffectorState(
            position=r[abi.MPPI_EE_POSITION:abi.MPPI_EE_POSITION + 3].copy(),
            orientation=r[abi.MPPI_EE_QUATERNION:abi.MPPI_EE_QUATERNION + 4].copy(),
            rotation=r[abi.MPPI_EE_ROTATION:abi.MPPI_EE_ROTATION + 9].reshape(3, 3).copy(),
            linear_velocity=r[abi.MPPI_EE_LINEAR_VELOCITY:abi.MPPI_EE_LINEAR_VELOCITY + 3].copy(),
            angular_velocity=r[abi.MPPI_EE_ANGULAR_VELOCITY:abi.MPPI_EE_ANGULAR_VELOCITY + 3].copy(),
            linear_acceleration=r[abi.MPPI_EE_LINEAR_ACCELERATION:abi.MPPI_EE_LINEAR_ACCELERATION + 3].copy(),
            angular_acceleration=r[abi.MPPI_EE_ANGULAR_ACCELERATION:abi.MPPI_EE_ANGULAR_ACCELERATION + 3].copy(),
            jacobian=r[abi.MPPI_EE_JACOBIAN:abi.MPPI_EE_JACOBIAN + 72].reshape(6, 12).copy())


class PinocchioDynamicsObject:
    """FrankaRidgeback::PinocchioDynamics (pinocchio_dynamics.hpp:30-427) on the device.
    `create(initial_state)` runs the constructor's set_state (pinocchio_dynamics.cpp:84-115)."""
    STATE_DOF = abi.MPPI_FR_STATE
    CONTROL_DOF = abi.MPPI_FR_CONTROL

    def __init__(self, handle, descriptor, link_positions=None, simulated_wrench=None):
        self._L = load()
        self._h = handle
        self._desc = descriptor
        self._link_positions = link_positions
        if link_positions is not None:
            self.set_link_positions(abi.MPPI_LINK_POSITIONS_KINEMATIC if link_positions else abi.MPPI_LINK_POSITIONS_ZERO)
        if simulated_wrench is not None:
            self.set_simulated_wrench(abi.MPPI_SIMULATED_WRENCH_ON if simulated_wrench else abi.MPPI_SIMULATED_WRENCH_OFF)

    @staticmethod
    def create(initial_state, model=None, device=0, link_positions=None, simulated_wrench=None):
        """`link_positions`: True the kinematic link-position model, False the reference's stub,
        None what MPPI_LINK_POSITIONS says (unset: the stub).  `simulated_wrench`: True forecast()
        applies its wrench rows, False it only copies them (the reference's stub), None what
        MPPI_SIMULATED_WRENCH says (unset: the stub)."""
        from .trajectory import EngineError, FrankaRidgebackDynamics
        L = load()
        desc = FrankaRidgebackDynamics(model).descriptor()
        x = np.ascontiguousarray(initial_state, dtype=np.float64).reshape(-1)
        if x.size != abi.MPPI_FR_STATE:
            raise ValueError("initial state must have %d entries" % abi.MPPI_FR_STATE)
        h = C.c_void_p()
        st = L.mppi_dynamics_create(C.byref(desc), _p(x), int(device), C.byref(h))
        if st != abi.MPPI_OK:
            raise EngineError(st, L.mppi_last_error(None).decode())
        return PinocchioDynamicsObject(h, desc, link_positions, simulated_wrench)

    def close(self):
        if getattr(self, "_h", None):
            self._L.mppi_dynamics_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != abi.MPPI_OK:
            from .trajectory import EngineError
            raise EngineError(st, self._L.mppi_last_error(None).decode())

    @property
    def handle(self):
        return self._h

    def copy(self):
        """mppi::Dynamics::copy (mppi.hpp:47): a new object at this one's state."""
        return PinocchioDynamicsObject.create(self.get_state(), link_positions=self._link_positions,
                                              simulated_wrench=self.simulated_wrench)

    def set_state(self, state, time):
        x = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        assert x.size == abi.MPPI_FR_STATE
        self._check(self._L.mppi_dynamics_set_state(self._h, _p(x), float(time)))

    def step(self, control, dt):
        """PinocchioDynamics::step (pinocchio_dynamics.cpp:226-260): the new state."""
        u = np.ascontiguousarray(control, dtype=np.float64).reshape(-1)
        assert u.size == abi.MPPI_FR_CONTROL
        out = np.zeros(abi.MPPI_FR_STATE)
        self._check(self._L.mppi_dynamics_step(self._h, _p(u), float(dt), _p(out)))
        return out

    def get_state(self):
        out = np.zeros(abi.MPPI_FR_STATE)
        self._check(self._L.mppi_dynamics_get_state(self._h, _p(out)))
        return out

    def get_end_effector_state_row(self):
        """The EndEffectorState as its MPPI_EE_N-double row."""
        out = np.zeros(abi.MPPI_EE_N)
        self._check(self._L.mppi_dynamics_end_effector(self._h, _p(out)))
        return out

    def get_end_effector_state(self):
        return EndEffectorState.from_row(self.get_end_effector_state_row())

    def set_link_positions(self, mode):
        """mppi_dynamics_set_link_positions (abi.MPPI_LINK_POSITIONS_*); evaluate_cost follows it."""
        self._check(self._L.mppi_dynamics_set_link_positions(self._h, int(mode)))
        self._link_positions = int(mode) == abi.MPPI_LINK_POSITIONS_KINEMATIC

    def add_end_effector_simulated_wrench(self, wrench):
        """PinocchioDynamics::add_end_effector_simulated_wrench: a force and a moment at the grasp
        frame's origin in world axes (6), cumulative; the next step applies the sum and zeroes it."""
        w = np.ascontiguousarray(wrench, dtype=np.float64).reshape(-1)
        assert w.size == 6
        self._check(self._L.mppi_dynamics_add_end_effector_simulated_wrench(self._h, _p(w)))

    def get_end_effector_simulated_wrench(self):
        """The wrench the last step applied (6); zeros before any step."""
        o = np.zeros(6)
        self._check(self._L.mppi_dynamics_get_end_effector_simulated_wrench(self._h, _p(o)))
        return o

    def safety_filter(self, filter, control, dt):
        """mppi_dynamics_safety_filter: the TrajectorySafetyFilter `filter` on one control (12) at the
        object's current joint position and velocity with time step `dt`; the filtered control.  A
        wrench added since the last step is included and not consumed."""
        u = np.ascontiguousarray(control, dtype=np.float64).reshape(-1)
        assert u.size == abi.MPPI_FR_CONTROL
        c = filter.to_c()
        out = np.zeros(abi.MPPI_FR_CONTROL)
        self._check(self._L.mppi_dynamics_safety_filter(self._h, C.byref(c), _p(u), float(dt), _p(out)))
        return out

    def set_simulated_wrench(self, mode):
        """mppi_dynamics_set_simulated_wrench (abi.MPPI_SIMULATED_WRENCH_OFF / _ON): whether
        forecast() adds its wrench rows before each step."""
        self._check(self._L.mppi_dynamics_set_simulated_wrench(self._h, int(mode)))

    @property
    def simulated_wrench(self):
        """Whether forecast() applies its wrench rows (mppi_dynamics_get_simulated_wrench)."""
        m = C.c_int(0)
        self._check(self._L.mppi_dynamics_get_simulated_wrench(self._h, C.byref(m)))
        return m.value == abi.MPPI_SIMULATED_WRENCH_ON

    def link_positions(self):
        """get_link_position of every Link (abi.LINK_NAMES order) after the last call, (13, 3): the
        body frames' world translations of the last calculate() in the kinematic model, zeros in
        the reference's stub."""
        o = np.zeros((abi.MPPI_LINK_N, 3))
        self._check(self._L.mppi_dynamics_link_positions(self._h, _p(o)))
        return o

    def get_link_position(self, link):
        return self.link_positions()[int(link)]

    def capsule_cost(self, config, capsules, obstacles, elapsed):
        """mppi_dynamics_capsule_cost: obstacle_cost with the robot's segments (`capsules`: an
        ObstacleCapsules or None, the defaults), capsule obstacles and segment mask bits."""
        from .obstacles import ObstacleAvoidance, ObstacleCapsules, obstacles_to_c
        c = (config or ObstacleAvoidance()).to_c()
        cc = (capsules or ObstacleCapsules()).to_c()
        arr, n = obstacles_to_c(obstacles)
        v = C.c_double(0.0)
        self._check(self._L.mppi_dynamics_capsule_cost(self._h, C.byref(c), C.byref(cc), arr, n, float(elapsed), C.byref(v)))
        return v.value

    def distance_field_cost(self, config, capsules, field):
        """mppi_dynamics_distance_field_cost: the distance field's term (Trajectory.set_distance_field)
        of `field` (a DistanceField) at the positions the object holds, with `config`'s limit and point
        radii and `capsules`' segment radii (None: the defaults).  The grid is uploaded on every call."""
        from .obstacles import ObstacleAvoidance, ObstacleCapsules
        c = (config or ObstacleAvoidance()).to_c()
        cc = (capsules or ObstacleCapsules()).to_c()
        f = field.to_c()
        v = C.c_double(0.0)
        self._check(self._L.mppi_dynamics_distance_field_cost(self._h, C.byref(c), C.byref(cc), C.byref(f), field.values_ptr(),
                                                              C.byref(v)))
        return v.value

    def held_object_cost(self, config, obstacles, elapsed, field, held):
        """mppi_dynamics_held_object_cost: the held term (Trajectory.set_held_object) of `held` (a
        HeldObject or None) at the grasp pose the object cached at its last call, against `obstacles`
        moved by `elapsed` seconds (their held mask bits) and against `field` (a DistanceField or None),
        with `config`'s limit (None: the defaults)."""
        from .obstacles import ObstacleAvoidance, obstacles_to_c
        c = (config or ObstacleAvoidance()).to_c()
        arr, n = obstacles_to_c(obstacles or [])
        f = field.to_c() if field is not None else None
        o = held.to_c() if held is not None else None
        v = C.c_double(0.0)
        self._check(self._L.mppi_dynamics_held_object_cost(self._h, C.byref(c), arr, n, float(elapsed),
                                                           C.byref(f) if f is not None else None,
                                                           field.values_ptr() if field is not None else None,
                                                           C.byref(o) if o is not None else None, C.byref(v)))
        return v.value

    def held_self_cost(self, config, held, held_self):
        """mppi_dynamics_held_self_cost: the held-self term (Trajectory.set_held_self) of `held` (a
        HeldObject or None) under `held_self` (a HeldSelf or None) at the link positions and the grasp
        pose the object cached at its last call, with `config`'s limit (None: the defaults).  Needs
        kinematic link positions."""
        from .obstacles import ObstacleAvoidance
        c = (config or ObstacleAvoidance()).to_c()
        o = held.to_c() if held is not None else None
        f = held_self.to_c() if held_self is not None else None
        v = C.c_double(0.0)
        self._check(self._L.mppi_dynamics_held_self_cost(self._h, C.byref(c), C.byref(o) if o is not None else None,
                                                         C.byref(f) if f is not None else None, C.byref(v)))
        return v.value

    def obstacle_cost(self, config, obstacles, elapsed):
        """mppi_dynamics_obstacle_cost: the obstacle term (Trajectory.set_obstacle_avoidance) of
        `obstacles` moved by `elapsed` seconds, at the link and end-effector positions the object
        cached at its last call.  `config`: an ObstacleAvoidance or None (the defaults).  The object
        must be in the kinematic link-position model."""
        from .obstacles import ObstacleAvoidance, obstacles_to_c
        c = (config or ObstacleAvoidance()).to_c()
        arr, n = obstacles_to_c(obstacles)
        v = C.c_double(0.0)
        self._check(self._L.mppi_dynamics_obstacle_cost(self._h, C.byref(c), arr, n, float(elapsed), C.byref(v)))
        return v.value

    def target_cost(self, point, quaternion=None, config=None):
        """mppi_dynamics_target_cost: the target-tracking terms (Trajectory.set_target_tracking) at the
        grasp frame's pose the object cached at its last call: (100 |p_EE - point|^2, weight (3 -
        sum_ij Rt_ij Ree_ij)), the second 0 without a `quaternion` (x, y, z, w; normalised by the
        engine).  `config`: a TargetTracking or None (the defaults)."""
        from .targets import TargetTracking
        c = (config or TargetTracking()).to_c()
        p = np.ascontiguousarray(point, dtype=np.float64).reshape(3)
        q = None if quaternion is None else np.ascontiguousarray(quaternion, dtype=np.float64).reshape(4)
        o = np.zeros(2)
        self._check(self._L.mppi_dynamics_target_cost(self._h, _p(p), None if q is None else _p(q), C.byref(c), _p(o)))
        return float(o[0]), float(o[1])

    def query_row(self):
        """The members after the last call as MPPI_DYNAMICS_QUERY_N doubles."""
        o = np.zeros(abi.MPPI_DYNAMICS_QUERY_N)
        self._check(self._L.mppi_dynamics_query(self._h, _p(o)))
        return o

    def query(self):
        """dict of the members after the last call: joint position / velocity / acceleration /
        torque, tank energy, power, time, arm-mount frame position."""
        o = self.query_row()
        return {"joint_position": o[0:12], "joint_velocity": o[12:24], "joint_acceleration": o[24:36],
                "joint_torque": o[36:48], "tank_energy": o[48], "power": o[49], "time": o[50],
                "arm_mount_position": o[51:54]}

    def get_joint_position(self):
        return self.query()["joint_position"]

    def get_joint_velocity(self):
        return self.query()["joint_velocity"]

    def get_tank_energy(self):
        return self.query()["tank_energy"]

    def get_joint_power(self):
        return 0.0   # pinocchio_dynamics.hpp:211-214

    def get_external_power(self):
        return 0.0   # pinocchio_dynamics.hpp:220-223

    def get_control_dof(self):
        return abi.MPPI_FR_CONTROL

    def get_state_dof(self):
        return abi.MPPI_FR_STATE

    def forecast_rows(self, state, time, time_step, steps, wrench=None):
        """[steps x MPPI_DF_N] rows of DynamicsForecast::forecast (mppi_dynamics_forecast)."""
        x = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
        out = np.zeros((int(steps), abi.MPPI_DF_N))
        w = None if wrench is None else np.ascontiguousarray(wrench, dtype=np.float64).reshape(int(steps), 6)
        self._check(self._L.mppi_dynamics_forecast(self._h, _p(x), float(time), float(time_step), int(steps),
                                                   None if w is None else _p(w), _p(out)))
        return out


def evaluate_cost(cost, dynamics, state, control=None, wrench=None):
    """Cost::get_cost(state, control, dynamics, time) (mppi.hpp:127-132) on the device against a
    PinocchioDynamicsObject's cached kinematics; `wrench` = forecast(time) of the dynamics' forecast
    handle (None: no handle, trajectory_cost 0).  Returns (cost, seven AssistedManipulation terms)."""
    L = load()
    desc = cost.descriptor()
    x = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
    u = np.zeros(abi.MPPI_FR_CONTROL) if control is None else np.ascontiguousarray(control, dtype=np.float64)
    w = None if wrench is None else np.ascontiguousarray(wrench, dtype=np.float64).reshape(6)
    out = np.zeros(8)
    st = L.mppi_cost_evaluate(C.byref(desc), dynamics.handle, _p(x), _p(u), None if w is None else _p(w), _p(out))
    if st != abi.MPPI_OK:
        from .trajectory import EngineError
        raise EngineError(st, L.mppi_last_error(None).decode())
    return out[0], out[1:]


class DynamicsForecast:
    """FrankaRidgeback::DynamicsForecast (dynamics.hpp:122-387, dynamics.cpp:57-138).  The wrench
    forecast it owns in the reference is the trajectory's device forecast here (`source`: a
    Trajectory with mppi_forecast_attach done, the forecast the rollouts' trajectory cost reads, as
    the Actor shares one DynamicsForecast between both, actor.cpp:70-89).  forecast() is one
    device launch for the whole horison."""

    def __init__(self, time_step, horison, dynamics, source):
        import math
        self.time_step, self.horison = float(time_step), float(horison)
        self.steps = int(math.ceil(horison / time_step))
        if self.steps <= 0:
            raise ValueError("time horison is too small for time step")   # dynamics.cpp:70-74
        self.dynamics = dynamics
        self.source = source
        self.last_forecast = np.finfo(np.float64).tiny   # std::numeric_limits<double>::min()
        self.rows = np.zeros((self.steps, abi.MPPI_DF_N))

    def observe_wrench(self, wrench, time):
        self.source.observe_wrench(wrench, time)

    def observe_time(self, time):
        self.source.observe_time(time)

    def forecast(self, state, time):
        wrench = self.source.forecast_table(time, self.time_step, self.steps)
        self.rows = self.dynamics.forecast_rows(state, time, self.time_step, self.steps, wrench)
        self.last_forecast = float(time)

    def get_last_forecast_time(self):
        return self.last_forecast

    def parameterise(self, time):
        """dynamics.hpp:344-359, literally (the horison is compared with the absolute time)."""
        if time < self.last_forecast:
            return 0
        if time >= self.horison:
            return self.steps - 1
        return int((time - self.last_forecast) / self.time_step)

    def get_joint_position(self):
        return self.rows[:, abi.MPPI_DF_JOINT_POSITION:abi.MPPI_DF_JOINT_POSITION + 12].copy()

    def get_end_effector_state(self, time):
        k = self.parameterise(time)
        return EndEffectorState.from_row(self.rows[k, abi.MPPI_DF_END_EFFECTOR:abi.MPPI_DF_END_EFFECTOR + abi.MPPI_EE_N])

    def get_end_effector_wrench(self, time):
        return self.source.forecast(time)   # dynamics.hpp:275-278: the forecast itself, not the rows

    def get_end_effector_trajectory(self):
        return [EndEffectorState.from_row(r[abi.MPPI_DF_END_EFFECTOR:abi.MPPI_DF_END_EFFECTOR + abi.MPPI_EE_N])
                for r in self.rows]

    def get_wrench_trajectory(self):
        return self.rows[:, abi.MPPI_DF_WRENCH:abi.MPPI_DF_WRENCH + 6].copy()

    def get_joint_power_trajectory(self):
        return self.rows[:, abi.MPPI_DF_JOINT_POWER].copy()

    def get_external_power_trajectory(self):
        return self.rows[:, abi.MPPI_DF_EXTERNAL_POWER].copy()

    def get_energy_trajectory(self):
        return self.rows[:, abi.MPPI_DF_ENERGY].copy()

    def get_time_step(self):
        return self.time_step

    def get_horison(self):
        return self.horison
