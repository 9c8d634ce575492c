"""GPU: posed joints and world joint rotations (moshii_joints_*) on the device -- the bodies and the checker of
tests/joints_common.py through the real library, at frame counts that are no multiple of a workgroup's waves and span many
workgroups; the cross-check against the full-mesh export, device buffers on a stream, a solved sequence, and two host threads."""
import threading

import numpy as np
import pytest

from tests import joints_common as jc
from tests import normals_common as nc

pytestmark = pytest.mark.gpu

BODIES = ('mano', 'smpl', 'smplh', 'smplx', 'horse', 'one', 'chain', 'star', 'pinned')


@pytest.mark.parametrize('name,F', [(n, 259) for n in BODIES] + [('smplh', 1), ('mano', 4097)])
def test_posed_joints_against_the_oracle(name, F):
    """259 frames: 64 full workgroups of four waves and one with three; 1 frame: three spare waves; 4097: beyond a thousand workgroups."""
    b = jc.body(name)
    dev = jc.device(b)
    jc.run_body(dev, b, F)
    dev.close()


@pytest.mark.parametrize('dtype,tol', [(np.float64, 2 * jc.F64_TOL), (np.float32, jc.F32_TOL)])
def test_pinned_body_export_vertices_are_the_joints(dtype, tol):
    """Vertex v_k of the merged full-mesh export is joint k, with the free block's coefficients; float32: the export's own bound."""
    b = jc.body('pinned')
    dev = jc.device(b)
    jc.check_pinned(dev, b, 259, True, dtype=dtype, tol=tol)
    jc.check_pinned(dev, b, 259, False, dtype=dtype, tol=tol)
    dev.close()


def _torch_stream_worker(rank):
    """In a process of its own, torch first: its HIP runtime finds no device once libmoshii's has initialised one in the same process
    (the project's torch users -- bench.py, workload.DeviceSequence, the RCCL test -- start that way too)."""
    import torch
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    from moshpp_amd import capi
    b = jc.body('smplx')
    dev = jc.device(b)
    F, K = 259, b['m']['K']
    for dtype in (np.float32, np.float64):
        pose, trans, shape = jc.inputs(b, F, dtype)
        isz = pose.itemsize
        bufs = [capi.DeviceBuffer(n) for n in (pose.nbytes, trans.nbytes, shape.nbytes, F * K * 3 * isz, F * K * 9 * isz)]
        bufs[0].upload(pose); bufs[1].upload(trans); bufs[2].upload(shape)
        for s in (None, shape):
            want_j, want_r = dev.posed_joints(pose, trans, shape=s, dtype=dtype, return_rotations=True)
            sp = None if s is None else bufs[2].ptr
            dev.posed_joints_device(F, bufs[0].ptr, bufs[1].ptr, bufs[3].ptr, rot_ptr=bufs[4].ptr, stream=stream.cuda_stream,
                                    f32=dtype == np.float32, shape_ptr=sp)
            stream.synchronize()
            assert capi.last_launch_info()[0] == jc.NAMES[(dtype, s is not None)]
            np.testing.assert_array_equal(bufs[3].download(np.zeros((F, K, 3), dtype=dtype)), want_j)
            np.testing.assert_array_equal(bufs[4].download(np.zeros((F, K, 3, 3), dtype=dtype)), want_r)
            bufs[3].upload(np.zeros((F, K, 3), dtype=dtype))                      # joints alone
            dev.posed_joints_device(F, bufs[0].ptr, bufs[1].ptr, bufs[3].ptr, stream=stream.cuda_stream, f32=dtype == np.float32, shape_ptr=sp)
            stream.synchronize()
            np.testing.assert_array_equal(bufs[3].download(np.zeros((F, K, 3), dtype=dtype)), want_j)
        for bf in bufs:
            bf.close()
    dev.close()


def test_device_buffers_on_a_torch_stream_equal_the_host_call():
    """posed_joints_device on capi.DeviceBuffers and a non-default torch stream: the host-buffer call's bits, both precisions, with and
    without a shape row, with and without rotations."""
    import torch.multiprocessing as mp
    mp.spawn(_torch_stream_worker, nprocs=1, join=True)


def test_joints_of_a_solved_sequence():
    """StageIISolver.joints after a short real SMPL-H solve (hand PCA on the solver's handle): the oracle's joints at the returned
    pose / trans; the root joint sits at J[0] + trans -- the root turns about its own joint."""
    from moshpp_amd import synth, workload
    from oracle import stageii_oracle as so
    dd = synth.synth_mesh_model('smplh', seed=1000, n_verts=1500)
    F, M = 24, 53
    job = workload.make_job('smplh', F, M, seed=1000, dd=dd)
    solver = workload.make_solver(job)
    out = solver.solve(np.asarray(job['obs'], dtype=np.float64), np.asarray(job['vis'], dtype=bool), chain_mode='sequential')
    assert (out['status'] != 1).all()
    joints, rot = solver.joints(out, return_rotations=True)
    sm = job['sm']
    assert sm.hand_dof > 0 and joints.shape == (F, sm.K, 3) and joints.dtype == np.float64
    model = dict(v_template=sm.v_template, shapedirs=sm.shapedirs, posedirs=sm.posedirs, weights=sm.weights, J_regressor=sm.J_regressor,
                 parents=sm.parents, body_dof=sm.body_dof, hand_dof=sm.hand_dof, hands_mean=sm.hands_mean,
                 selected_components=sm.selected_components)
    m = so.prepare_model(model, job['betas'])
    pose, trans = np.ascontiguousarray(out['pose'], dtype=np.float64), np.ascontiguousarray(out['trans'], dtype=np.float64)
    jc.check(joints, rot, m, pose, trans, None, np.float64)
    root = np.abs(joints[:, 0] - (solver.dev.joints()[0] + trans)).max()
    print(f'root joint vs J[0] + trans: {root:.3e}')
    assert root <= jc.F64_TOL
    np.testing.assert_array_equal(solver.joints(out), joints)
    j32 = solver.joints(out, dtype=np.float32)
    jc.check(j32, None, m, pose.astype(np.float32), trans.astype(np.float32), None, np.float32)


def test_two_threads_joints_and_export_on_two_handles():
    """posed_joints on one handle while lbs_forward runs on another, each from its own host thread; both results pass their checks."""
    b1, b2 = jc.body('smplh'), jc.body('smpl')
    d1, d2 = jc.device(b1), jc.device(b2)
    F = 259
    pose1, trans1, _ = jc.inputs(b1, F, np.float64)
    pose2, trans2 = nc.inputs(nc.mesh_case('smpl', 1500), 16)
    ref1 = jc.oracle(b1['m'], pose1, trans1)
    ref2 = nc.oracle_verts(b2['m'], pose2, trans2)
    got, errs = {}, []

    def joints_loop():
        try:
            for i in range(8):
                got[('j', i)] = d1.posed_joints(pose1, trans1, return_rotations=True)
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    def export_loop():
        try:
            for i in range(8):
                got[('v', i)] = d2.lbs_forward(pose2, trans2)
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=joints_loop), threading.Thread(target=export_loop)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for i in range(8):
        j, r = got[('j', i)]
        if i == 0:
            jc.check(j, r, b1['m'], pose1, trans1, None, np.float64, ref=ref1)
        else:
            np.testing.assert_array_equal(j, got[('j', 0)][0])
            np.testing.assert_array_equal(r, got[('j', 0)][1])
        assert np.abs(got[('v', i)] - ref2).max() < jc.F64_TOL
    d1.close(); d2.close()
