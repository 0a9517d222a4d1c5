"""External collisions from joint torques: a numpy transcription of the reference's classes, the yardstick of wbcqp_detect_torque_collisions.

    Filter / MovingAverageFilter / MedianFilter    include/inria_wbc/estimators/filtering.hpp there, growth phase included
    TorqueCollisionDetection                        src/safety/torque_collision_detection.cpp there: check() with its ring of signs, as written
    detect(monitor, tau_model, tau_sensor, state)   the classes over [T][B][.] arrays, every instance's joints as variables of one detector
    shift_register_invalid                          the form the kernel keeps (two K-bit registers per joint), for comparison with the ring of signs
    TALOS_JOINTS, TALOS_THRESHOLDS, read_thresholds what TalosPosTracker::parse_torque_safety sets up (src/controllers/talos_pos_tracker.cpp:62-123)

Everything here runs on the host in double precision and is deliberately slow and literal.  Monitor also describes a monitor to the library
(capi.Handle.detect_torque_collisions).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

FILTER_NONE, FILTER_MEAN, FILTER_MEDIAN = 0, 1, 2
MAX_MONITORED, MAX_FILTER_WINDOW, MAX_INVALID = 64, 64, 31

# the 22 joints the reference's Talos controller monitors and its default thresholds (talos_pos_tracker.cpp:71-89)
TALOS_JOINTS = (
    "leg_left_1_joint", "leg_left_2_joint", "leg_left_3_joint", "leg_left_4_joint", "leg_left_5_joint", "leg_left_6_joint",
    "leg_right_1_joint", "leg_right_2_joint", "leg_right_3_joint", "leg_right_4_joint", "leg_right_5_joint", "leg_right_6_joint",
    "torso_1_joint", "torso_2_joint",
    "arm_left_1_joint", "arm_left_2_joint", "arm_left_3_joint", "arm_left_4_joint",
    "arm_right_1_joint", "arm_right_2_joint", "arm_right_3_joint", "arm_right_4_joint")
TALOS_THRESHOLDS = (3.5e+05, 3.9e+05, 2.9e+05, 4.4e+05, 5.7e+05, 2.4e+05,
                    3.5e+05, 3.9e+05, 2.9e+05, 4.4e+05, 5.7e+05, 2.4e+05,
                    1e+01, 1e+01,
                    1e+01, 1e+01, 1e+01, 1e+01,
                    1e+01, 1e+01, 1e+01, 1e+01)


class Filter:
    """Filter (filtering.hpp:17-101): a buffer [nvar][wsize] that fills from the left and then shifts left by one column per sample."""

    def __init__(self, nvar: int, wsize: int):
        self._nvar, self._wsize = int(nvar), int(wsize)
        self.reset()

    def reset(self) -> None:
        self._buffer = np.zeros((self._nvar, self._wsize))
        self._filtered = np.zeros(self._nvar)
        self._cnt = 0

    def data_ready(self) -> bool:
        return self._cnt >= self._wsize

    def filter(self, sample: np.ndarray) -> np.ndarray:
        sample = np.asarray(sample, dtype=np.float64)
        assert sample.shape == (self._nvar,), "Size of sample differs from filter get_num_var()!"
        if self._cnt < self._wsize:
            self._buffer[:, self._cnt] = sample
            self._cnt += 1
            self._filter_impl(self._buffer[:, :self._cnt])
        else:
            if self._wsize > 1:
                self._buffer[:, :self._wsize - 1] = self._buffer[:, 1:].copy()
            self._buffer[:, -1] = sample
            self._filter_impl(self._buffer)
        return self._filtered

    def _filter_impl(self, window: np.ndarray) -> None:
        raise NotImplementedError


class MovingAverageFilter(Filter):
    """window.rowwise().mean(): the columns summed oldest first, one division by their number."""

    def _filter_impl(self, window: np.ndarray) -> None:
        total = np.zeros(window.shape[0])
        for c in range(window.shape[1]):
            total = total + window[:, c]
        self._filtered = total / float(window.shape[1])


class MedianFilter(Filter):
    """The middle element of each sorted row; (v[c/2] + v[c/2-1]) / 2 for an even count.  (np.sort puts NaNs last.)"""

    def _filter_impl(self, window: np.ndarray) -> None:
        c = window.shape[1]
        v = np.sort(window, axis=1)  # every row on its own, as the loop over rows there
        self._filtered = (v[:, c // 2] + v[:, c // 2 - 1]) / 2 if c % 2 == 0 else v[:, c // 2].copy()


def _sign(d: np.ndarray) -> np.ndarray:
    """Eigen's sign() cast to int; a NaN has no sign here (that cast is undefined in the reference)."""
    return (d > 0).astype(np.int64) - (d < 0).astype(np.int64)


class TorqueCollisionDetection:
    """safety::TorqueCollisionDetection, member for member where the result depends on it."""

    def __init__(self, threshold: Sequence[float]):
        self._threshold = np.asarray(threshold, dtype=np.float64).reshape(-1).copy()
        self._nvar = self._threshold.size
        self._step_count = 0
        self._offset, self._add_offset = np.zeros(self._nvar), False
        self._filter: Optional[Filter] = None
        self._discrepancy = np.zeros(self._nvar)
        self._filtered_sensors = np.zeros(self._nvar)
        self._validity = np.ones(self._nvar, dtype=bool)
        self.set_max_consecutive_invalid(0)

    def set_max_consecutive_invalid(self, counter: int) -> None:
        self._invalid_threshold = int(counter) + 1
        self._previous_signs = np.zeros((self._nvar, self._invalid_threshold), dtype=np.int64)

    def set_threshold(self, threshold) -> None:
        t = np.asarray(threshold, dtype=np.float64)
        self._threshold = np.full(self._nvar, float(t)) if t.ndim == 0 else t.reshape(self._nvar).copy()

    def set_offset(self, offset) -> None:
        self._offset, self._add_offset = np.asarray(offset, dtype=np.float64).reshape(self._nvar).copy(), True

    def remove_offset(self) -> None:
        self._offset, self._add_offset = np.zeros(self._nvar), False

    def set_filter(self, f: Optional[Filter]) -> None:
        self._filter = f

    def reset(self) -> None:
        self._step_count = 0
        self._previous_signs[:] = 0
        if self._filter is not None:
            self._filter.reset()

    def check(self, target: np.ndarray, sensors: np.ndarray) -> bool:
        self._step_count += 1
        sensors = np.asarray(sensors, dtype=np.float64)
        self._filtered_sensors = np.array(self._filter.filter(sensors) if self._filter is not None else sensors, dtype=np.float64)
        if self._add_offset:
            self._filtered_sensors = self._filtered_sensors + self._offset
        # _compute_validity
        self._discrepancy = np.asarray(target, dtype=np.float64) - self._filtered_sensors
        self._validity = np.abs(self._discrepancy) < self._threshold
        # _compute_validity_over_steps (_invalid_threshold = counter + 1 is never 0)
        if self._invalid_threshold > 0:
            nval = 1 - self._validity.astype(np.int64)
            self._previous_signs[:, self._step_count % self._invalid_threshold] = nval * _sign(self._discrepancy)
            cumulated = np.abs(self._previous_signs.sum(axis=1))
            self._validity = cumulated < self._invalid_threshold
        return bool(self._validity.all())

    def get_discrepancy(self) -> np.ndarray:
        return self._discrepancy

    def get_filtered_sensors(self) -> np.ndarray:
        return self._filtered_sensors

    def get_validity(self) -> np.ndarray:
        return self._validity.astype(np.int32)

    def get_invalid_ids(self) -> List[int]:
        return [i for i in range(self._nvar) if not self._validity[i]]


@dataclass
class Monitor:
    """A wbcqp_torque_monitor: which columns of a tau_model row are monitored, against which thresholds, through which filter."""
    joint: Sequence[int]
    threshold: Sequence[float]
    offset: Optional[Sequence[float]] = None
    filter: int = FILTER_MEAN
    window: int = 30
    max_invalid: int = 5

    @property
    def n_joints(self) -> int:
        return len(self.joint)

    def state_bytes(self) -> int:
        """Bytes of one instance's state in the library (wbcqp_torque_monitor_state_bytes computes the same)."""
        return 8 + 8 * self.n_joints + (0 if self.filter == FILTER_NONE else 8 * self.window * self.n_joints)

    def detector(self, instances: int = 1) -> TorqueCollisionDetection:
        """A fresh detector of the reference's, set up as this monitor says.  instances > 1: ONE detector whose variables are the joints of that many
        instances side by side -- the reference's classes treat every variable on its own, so this is `instances` detectors run in step."""
        nvar = self.n_joints * instances
        d = TorqueCollisionDetection(np.tile(np.asarray(self.threshold, dtype=np.float64), instances))
        d.set_max_consecutive_invalid(self.max_invalid)
        if self.filter == FILTER_MEAN:
            d.set_filter(MovingAverageFilter(nvar, self.window))
        elif self.filter == FILTER_MEDIAN:
            d.set_filter(MedianFilter(nvar, self.window))
        if self.offset is not None:
            d.set_offset(np.tile(np.asarray(self.offset, dtype=np.float64), instances))
        return d


def detect(monitor: Monitor, tau_model: np.ndarray, tau_sensor: np.ndarray, state: Optional[TorqueCollisionDetection] = None) -> dict:
    """The reference's detector over tau_model [T][B][ldt] and tau_sensor [T][B][n_joints].  `state`: the detector a previous call returned under
    "state" (None: a fresh one, Monitor.detector(B)).  Returns what wbcqp_torque_checks holds, in double, and the detector."""
    tau_model, tau_sensor = np.asarray(tau_model, dtype=np.float64), np.asarray(tau_sensor, dtype=np.float64)
    T, B, n = tau_sensor.shape
    assert n == monitor.n_joints and tau_model.shape[:2] == (T, B)
    cols = np.asarray(monitor.joint, dtype=np.int64)
    det = state if state is not None else monitor.detector(B)
    assert det._nvar == B * n
    bit = np.left_shift(np.uint64(1), np.arange(n, dtype=np.uint64))
    out = {"detected": np.zeros((T, B), np.int32), "invalid": np.zeros((T, B), np.uint64), "discrepancy": np.zeros((T, B, n)),
           "filtered": np.zeros((T, B, n)), "first_tick": np.full(B, -1, np.int32), "n_detected": np.zeros(B, np.int32), "state": det}
    for t in range(T):
        det.check(tau_model[t][:, cols].reshape(B * n), tau_sensor[t].reshape(B * n))
        invalid = det.get_validity().reshape(B, n) == 0
        out["invalid"][t] = np.where(invalid, bit[None, :], np.uint64(0)).sum(axis=1, dtype=np.uint64)
        out["detected"][t] = invalid.any(axis=1)  # per instance: check() returned false
        out["discrepancy"][t] = det.get_discrepancy().reshape(B, n)
        out["filtered"][t] = det.get_filtered_sensors().reshape(B, n)
    hit = out["detected"] != 0
    out["n_detected"][:] = hit.sum(axis=0)
    out["first_tick"][:] = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
    return out


def shift_register_invalid(discrepancy: np.ndarray, threshold: np.ndarray, max_invalid: int) -> np.ndarray:
    """The consecutive rule as the kernel keeps it, on discrepancy [T][n]: two K-bit shift registers per joint (raw-invalid with d > 0, with d < 0),
    invalid iff |popcount(pos) - popcount(neg)| >= K.  Returns bool [T][n]."""
    d = np.asarray(discrepancy, dtype=np.float64)
    K = int(max_invalid) + 1
    mask = (1 << K) - 1
    pos = np.zeros(d.shape[1], dtype=np.uint64)
    neg = np.zeros(d.shape[1], dtype=np.uint64)
    out = np.zeros(d.shape, dtype=bool)
    popcount = np.vectorize(lambda x: bin(int(x)).count("1"), otypes=[np.int64])
    for t in range(d.shape[0]):
        raw_invalid = ~(np.abs(d[t]) < threshold)
        pos = ((pos << np.uint64(1)) | (raw_invalid & (d[t] > 0)).astype(np.uint64)) & np.uint64(mask)
        neg = ((neg << np.uint64(1)) | (raw_invalid & (d[t] < 0)).astype(np.uint64)) & np.uint64(mask)
        out[t] = np.abs(popcount(pos) - popcount(neg)) >= K
    return out


def read_thresholds(path: str, joints: Sequence[str] = TALOS_JOINTS, defaults: Sequence[float] = TALOS_THRESHOLDS) -> np.ndarray:
    """parse_collision_thresholds (talos_pos_tracker.cpp:113-123): `joint: value` lines of a flat settings file replace the defaults of the joints
    they name; other keys are ignored."""
    thr = np.asarray(defaults, dtype=np.float64).copy()
    index = {j: k for k, j in enumerate(joints)}
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line or ":" not in line:
                continue
            key, val = (s.strip() for s in line.split(":", 1))
            if key in index:
                thr[index[key]] = float(val)
    return thr
