"""The ONE table of cases behind tests/test_box_ref_cpu.py (which proves on the host that every case can tell a wrong heading from a
right one) and tests/test_gpu_axes.py (which runs the same cases on the device): BEV axis conventions, the shipped BEV configs, the
similarity matrices and the tracker-step inputs built from them.  Test infrastructure only."""
import os

import numpy as np
import yaml

from bev_amd.bevspec import BEVWorldSpec
from bev_amd.calib import Calib
from bev_amd.constructor import homo_constr

# every legal (u_axis, v_axis): the first four turn the raster into the world (det H > 0), the last four mirror it (det H < 0)
CONVENTIONS = [("x", "y"), ("-x", "-y"), ("y", "-x"), ("-y", "x"), ("x", "-y"), ("-x", "y"), ("y", "x"), ("-y", "-x")]
CONVENTION_IDS = ["u%s_v%s" % (u.replace("-", "m"), v.replace("-", "m")) for u, v in CONVENTIONS]
# the BEV configs the package ships (bev_amd/constructor/configs_bspec); the three "_3" cameras look the other way: mirrors
SHIPPED = ["0", "4_1", "4_2", "4_3", "5_1", "5_2", "5_3", "6_1", "6_2", "6_3"]
MIRRORED_SHIPPED = {"4_3", "5_3", "6_3"}
MULTIPLIERS = [1.0, -2.5]  # a homography is defined up to a factor: H[2][2] need not be 1, nor positive

# the tracker-step cases: (id, kind, key)
TRACKER_CASES = [("conv-" + i, "convention", c) for i, c in zip(CONVENTION_IDS, CONVENTIONS)] + [("brno-" + s, "shipped", s) for s in SHIPPED]
TRACKER_IDS = [c[0] for c in TRACKER_CASES]
N_DETS, N_TRKS = 130, 129
JITTER = (0.4, 0.4, 0.05, 0.1, 0.05)
GATE = {np.float64: 0.3, np.float32: 0.25}  # (0.25 is a float32: the gate reads the same in both precisions)
MIN_GATED, MIN_OVERLAPPING = 50, 150


def calib():
    """The camera of tests/test_gpu_geom.py::_tracker_case."""
    return Calib(vp1=np.array([1200.0, -300.0]), vp2=np.array([-2500.0, -150.0]), pp=np.array([959.5, 539.5]), height=8, u_size=1920, v_size=1080)


def convention_spec(u_axis, v_axis):
    """A 384 x 512 raster at 1 / 16 m per pixel, centred under the camera's image centre, with the given axes."""
    cfg = {"mode": "centered", "spec": {"u_axis": u_axis, "v_axis": v_axis, "u_size": 384, "v_size": 512, "m_per_px": 0.0625}}
    return homo_constr.load_bspec_from_cfg(cfg, calib())


def shipped_cfg(name):
    path = os.path.join(os.path.dirname(os.path.abspath(homo_constr.__file__)), "configs_bspec", "BrnoCompSpeed_%s.yaml" % name)
    with open(path) as f:
        return yaml.safe_load(f)


def shipped_spec(name):
    return homo_constr.load_bspec_from_cfg(shipped_cfg(name), calib())


def spec_of(kind, key):
    return convention_spec(*key) if kind == "convention" else shipped_spec(key)


def small_last_row(H, row=(3e-6, -2e-6)):
    """H normalised, with a last row that is small but not zero: inside the 1e-5 the transforms accept, so the divide by W is live."""
    Hn = np.array(H, dtype=np.float64) / H[2, 2]
    Hn[2, 0], Hn[2, 1] = row
    return Hn


def random_boxes_bev(rng, spec, n, scale):
    """n detections anywhere in the raster: cars of 1.6-2.2 m x 3.5-6 m at `scale` metres per pixel."""
    return np.column_stack([rng.uniform(0, spec.u_size, n), rng.uniform(0, spec.v_size, n), rng.uniform(1.6, 2.2, n) / scale,
                            rng.uniform(3.5, 6, n) / scale, rng.uniform(-np.pi, np.pi, n)])


def tracker_case(kind, key, dtype=np.float64, n=N_DETS, m=N_TRKS, seed=21):
    """Inputs of one tracker step, the construction of tests/test_gpu_geom.py::_tracker_case under another BEV spec: n detections in
    the raster, m tracker rows of 7 columns -- the first min(n, m, max(1, 2 m / 3)) are the detections' own world boxes, jittered, the
    rest lie anywhere in the world window.  The inputs are rounded to `dtype` (and returned as float64 arrays holding those values):
    the reference then sees exactly what the device sees."""
    from bev_amd import rbox as host_rbox
    spec = spec_of(kind, key)
    cal = calib()
    H_world_bev = spec.gen_H_world_bev()
    H_img_world = np.linalg.inv(cal.gen_H_world_img())
    Hn = H_world_bev / H_world_bev[2, 2]
    scale = np.hypot(Hn[0, 0], Hn[1, 0])
    rng = np.random.default_rng(seed)
    dets_bev = random_boxes_bev(rng, spec, n, scale).astype(dtype).astype(np.float64)
    k = min(n, m, max(1, (2 * m) // 3))
    near = host_rbox.rbox_world_bev(dets_bev[:k], H_world_bev, "bev") + rng.normal(0, JITTER, (k, 5))
    far = np.column_stack([rng.uniform(spec.x_min, spec.x_max, m - k), rng.uniform(spec.y_min, spec.y_max, m - k), rng.uniform(1.6, 2.2, m - k),
                           rng.uniform(3.5, 6, m - k), rng.uniform(-np.pi, np.pi, m - k)])
    trks = np.column_stack([np.vstack([near, far]), rng.normal(0, 1, (m, 2))]).astype(dtype).astype(np.float64)
    return {"dets_bev": dets_bev, "trks": trks, "H_world_bev": H_world_bev, "H_img_world": H_img_world, "spec": spec, "dtype": dtype,
            "threshold": GATE[dtype]}


def non_vacuity(exp_iou, threshold):
    """(pairs above the gate, pairs that overlap at all) of an expected IoU matrix, and the two floors every case must clear."""
    gated, overlapping = int((exp_iou > threshold).sum()), int((exp_iou > 0).sum())
    return gated, overlapping, gated >= MIN_GATED and overlapping >= MIN_OVERLAPPING
