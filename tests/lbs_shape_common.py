"""Shared by the full-mesh export tests with a free shape block (tests/test_lbs_shape_emulation.py, tests/test_gpu_lbs_shape.py):
bodies that carry E free shapedirs columns [16, 16 + E) -- helpers.shape_case's recipe for any model type and vertex order --
random export inputs, and the oracle's vertices for them."""
import numpy as np

from moshpp_amd import synth
from oracle import stageii_oracle as so
from tests.helpers import device_case, oracle_case

START = 16
MARKERS = {'smpl': 41, 'smplh': 53, 'smplx': 60, 'mano': 24}
F64_TOL = 1e-12      # the f64 kernel against the oracle: what tests/test_gpu_parity.py::test_lbs_f64_matches_oracle asks
F32_TOL = 2e-5       # the f32 export against reference precision (include/moshii.h)


def block_case(model_type, E, seed=61, order='shuffled'):
    """oracle_case whose model has E extra shapedirs columns, each scaled so that a unit coefficient moves its most affected vertex
    coordinate by 1 cm; the oracle model has the block declared (so.set_free_shape).  The frozen betas of those columns stay whatever
    the synthetic subject drew: the coefficients are an offset on them."""
    NB = START + E
    dd = dict(synth.synth_model(model_type, seed=seed, num_betas=NB, vertex_order=order))
    sd = np.array(dd['shapedirs'], dtype=np.float64)
    sd[:, :, START:] *= 0.01 / np.maximum(np.abs(sd[:, :, START:]).max(axis=(0, 1), keepdims=True), 1e-12)
    dd['shapedirs'] = sd
    case = oracle_case(model_type, F=4, M=MARKERS[model_type], seed=seed, num_betas=NB, dd=dd)
    so.set_free_shape(case['m'], START, E)
    case['E'], case['start'] = E, START
    return case


def block_device(case):
    dev = device_case(case)
    dev['model'].set_free_shape(case['start'], case['E'])
    return dev


def export_inputs(case, F, seed=5, still=None, amp=1.2):
    """pose N(0, 0.35), trans N(0, 1) as in the existing export tests; coefficients N(0, amp).  still: the pose variables from that
    index on are those of frame 0 in every frame."""
    rng = np.random.default_rng(seed)
    pose = rng.normal(0, 0.35, (F, case['m']['NP']))
    trans = rng.normal(0, 1, (F, 3))
    shape = rng.normal(0, amp, (F, case['E']))
    if still is not None:
        pose[:, still:] = pose[0, still:]
    return pose, trans, shape


def oracle_verts(m, pose, trans, shape=None):
    return np.stack([so.verts_forward(m, so.fullpose_from_pose(m, pose[f]), trans[f], shp=None if shape is None else shape[f])
                     for f in range(pose.shape[0])])
