"""CPU: who owns device memory in the model, prior and attach handles and in the export entries (moshpp_amd/csrc/dev_mem.h) -- in the
emulation build, whose stand-in runtime counts hipMalloc calls and live allocations and fails the n-th hipMalloc on request.

For every entry below and EVERY allocation of one good call: the call fails with MOSHII_ERR_HIP, nothing it allocated is left, a
handle keeps no half-built table, and the same call made again gives the bits of the untroubled call.  The sibling of
tests/test_chain_emulation.py::test_a_failed_allocation_frees_what_the_call_allocated_in_emulation, which covers the two solve entries.

Body: MANO at 778 vertices, F = 2 frames, M = 3 markers, N = 4 points -- the smallest body the emulation tests build."""
import ctypes as C

import numpy as np
import pytest

from tests import normals_common as nc
from tests.emu.emu_moshii import emulated_libmoshii

F, M, N, E = 2, 3, 4, 3          # frames, markers, points a frame, free shape coefficients
HIP_ERROR = r'libmoshii error -2:'   # MOSHII_ERR_HIP


class Bench:
    """One emulated library with its counters, a body and the inputs every entry shares."""

    def __init__(self, capi):
        self.capi = capi
        self.lib = capi.load()
        self.lib.hipemu_malloc_calls.restype = self.lib.hipemu_live_allocs.restype = C.c_long
        self.lib.hipemu_fail_malloc_in.argtypes = [C.c_long]
        self.case = nc.mesh_case('mano', 778)
        self.pose, self.trans = nc.inputs(self.case, F)
        rng = np.random.default_rng(9)
        self.shape = rng.normal(0, 1.0, (F, E))
        V = self.case['model']['v_template'].shape[0]
        self.vids = np.array([3, V // 2, V - 1], dtype=np.int32)
        self.dist = np.array([0.01, 0.0, 0.02])
        self.closest = rng.integers(0, V, (M, 3)).astype(np.int32)
        self.coef = rng.dirichlet(np.ones(3), M)
        self.betas = rng.normal(0, 0.5, self.case['model']['shapedirs'].shape[-1])

    def model(self, faces='case', block=True):
        dev = nc.device_model(self.case, faces=faces)
        if block:
            dev.set_free_shape(0, E)
        return dev

    def live(self):
        return self.lib.hipemu_live_allocs()

    def mallocs(self, fn):
        """(result, hipMalloc calls) of fn()."""
        before = self.lib.hipemu_malloc_calls()
        res = fn()
        return res, self.lib.hipemu_malloc_calls() - before

    def failing(self, nth, fn):
        self.lib.hipemu_fail_malloc_in(nth)
        try:
            with pytest.raises(self.capi.MoshiiError, match=HIP_ERROR):
                fn()
        finally:
            self.lib.hipemu_fail_malloc_in(0)

    def points(self, dev, dtype):
        v = dev.lbs_forward(self.pose, self.trans, dtype=dtype)
        return v, (v[:, :N] + np.random.default_rng(4).normal(0, 0.02, (F, N, 3))).astype(dtype)


def same(a, b):
    a, b = (x if isinstance(x, (tuple, list)) else (x,) for x in (a, b))
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def sd_tuple(r):
    return r.distance, r.face, r.part, r.nearest


def host_entries(b, dev):
    """name -> call on host buffers of a prepared handle, every optional output asked for (the issue's list)."""
    out = {}
    for dt, nm in ((np.float32, 'f32'), (np.float64, 'f64')):
        v, pts = b.points(dev, dt)
        out[f'lbs_forward_{nm}'] = lambda dt=dt: dev.lbs_forward(b.pose, b.trans, dtype=dt, shape=b.shape)
        out[f'vertex_normals_{nm}'] = lambda v=v: dev.vertex_normals(v)
        out[f'virtual_markers_{nm}'] = lambda dt=dt: dev.virtual_markers(b.pose, b.trans, b.vids, b.dist, dtype=dt, return_normals=True)
        out[f'surface_distance_{nm}'] = lambda v=v, pts=pts: sd_tuple(dev.surface_distance(v, pts))
        out[f'marker_surface_distance_{nm}'] = lambda dt=dt, pts=pts: sd_tuple(dev.marker_surface_distance(b.pose, b.trans, pts, dtype=dt))
        out[f'joints_{nm}'] = lambda dt=dt: dev.posed_joints(b.pose, b.trans, dtype=dt, return_rotations=True)
    return out


# hipMalloc calls of one host-buffer call before the entries shared an owner (measured on the emulation build of that commit with this
# file's host_entries): the inputs and outputs of the call, one each; no entry may make more.
PARENT_HOST_MALLOCS = {
    'lbs_forward_f32': 4, 'lbs_forward_f64': 4,                      # pose, trans, shape, verts
    'vertex_normals_f32': 2, 'vertex_normals_f64': 2,                # verts, normals
    'virtual_markers_f32': 4, 'virtual_markers_f64': 4,              # pose, trans, markers, normals
    'surface_distance_f32': 6, 'surface_distance_f64': 6,            # verts, points, dist, face, part, nearest
    'marker_surface_distance_f32': 7, 'marker_surface_distance_f64': 7,   # pose, trans, points, dist, face, part, nearest
    'joints_f32': 4, 'joints_f64': 4,                                # pose, trans, joints, rot
}


@pytest.fixture(scope='module')
def bench():
    with emulated_libmoshii() as capi:
        yield Bench(capi)


@pytest.mark.parametrize('name', sorted(PARENT_HOST_MALLOCS))
def test_host_buffer_entry_frees_its_temporaries_whichever_allocation_fails(bench, name):
    b = bench
    dev = b.model()
    try:
        call = host_entries(b, dev)[name]
        first = call()                               # (the scratch kept with the handle and the f32 copy have their size from here on)
        again, n = b.mallocs(call)
        print(name, 'hipMalloc calls of one host-buffer call:', n, 'before:', PARENT_HOST_MALLOCS[name])
        assert same(again, first)
        assert 1 <= n <= PARENT_HOST_MALLOCS[name]
        for nth in range(1, n + 1):
            live = b.live()
            b.failing(nth, call)
            assert b.live() == live, (nth, n)
            assert same(call(), first), nth
            assert b.live() == live, (nth, n)
    finally:
        dev.close()


def _prior_arrays():
    rng = np.random.default_rng(3)
    G, npose = 2, 5
    chols = np.tril(rng.normal(0, 1, (G, npose, npose))) + 3 * np.eye(npose)
    return rng.normal(0, 1, (G, npose)), chols, np.array([0.4, 0.6])


def test_create_entries_leave_nothing_of_the_handle_whichever_allocation_fails(bench):
    """moshii_model_create, moshii_prior_create, moshii_attach_create: a failure frees the handle and every array already uploaded."""
    b = bench
    dev = b.model()
    try:
        def model():
            m = b.model(faces=None, block=False)
            try:
                return m.joints()
            finally:
                m.close()

        def prior():
            b.capi.Prior(*_prior_arrays()).close()
            return np.zeros(1)

        def attach():
            a = b.capi.Attachment(dev, b.closest, b.coef)
            try:
                return a.markers(b.pose, b.trans)
            finally:
                a.close()

        for name, create in (('model_create', model), ('prior_create', prior), ('attach_create', attach)):
            live = b.live()
            first, n = b.mallocs(create)
            print(name, 'hipMalloc calls of create (+ one use) and destroy:', n)
            assert b.live() == live and n >= 5, name
            failed = 0
            for nth in range(1, n + 1):
                b.lib.hipemu_fail_malloc_in(nth)
                try:
                    create()                         # (the last allocations of `n` belong to the use, not to create: they raise too)
                except b.capi.MoshiiError as e:
                    assert 'libmoshii error -2:' in str(e), (name, nth, e)
                    failed += 1
                finally:
                    b.lib.hipemu_fail_malloc_in(0)
                assert b.live() == live, (name, nth, n)
                assert same(create(), first), (name, nth)
                assert b.live() == live, (name, nth, n)
            assert failed == n, (name, failed, n)
    finally:
        dev.close()


def test_set_betas_owns_its_temporary(bench):
    b = bench
    dev = b.model()
    try:
        def call():
            dev.set_betas(b.betas)
            return dev.joints()
        first, n = b.mallocs(call)
        assert n == 1
        live = b.live()
        b.failing(1, call)
        assert b.live() == live
        assert same(call(), first) and b.live() == live
    finally:
        dev.close()


def test_attach_markers_frees_its_temporaries_whichever_allocation_fails(bench):
    b = bench
    dev = b.model()
    att = b.capi.Attachment(dev, b.closest, b.coef)
    try:
        def call():
            return att.markers(b.pose, b.trans)
        first, n = b.mallocs(call)
        assert n == 3                                # pose, trans, markers
        for nth in range(1, n + 1):
            live = b.live()
            b.failing(nth, call)
            assert b.live() == live, nth
            assert same(call(), first) and b.live() == live, nth
    finally:
        att.close()
        dev.close()


def test_a_failed_set_faces_leaves_no_table(bench):
    """... never half of one: the handle had faces, the failed call leaves it without any (the three arrays of the old table are
    released, nothing of the new one stays), vertex_normals is refused, and the call made again restores the table."""
    b = bench
    dev = b.model()
    try:
        faces = b.case['faces']
        v = dev.lbs_forward(b.pose, b.trans)

        def call():
            dev.set_faces(faces)
            return dev.vertex_normals(v)
        first, n = b.mallocs(call)
        n -= 2                                       # (vertex_normals on host buffers: 2)
        assert n == 3                                # rows, pairs, triangles
        for nth in range(1, n + 1):
            live = b.live()
            b.failing(nth, lambda: dev.set_faces(faces))
            assert b.live() == live - 3, nth
            with pytest.raises(b.capi.MoshiiError, match='the model has no faces: call moshii_model_set_faces first'):
                dev.vertex_normals(v)
            assert same(call(), first) and b.live() == live, nth
    finally:
        dev.close()


def test_a_failed_set_free_shape_leaves_no_block(bench):
    """The handle had a block; the failed call leaves it with none -- no stale size beside a null pointer: a shape export is refused --
    and the call made again restores it."""
    b = bench
    dev = b.model()
    try:
        frozen = dev.lbs_forward(b.pose, b.trans)

        def call():
            dev.set_free_shape(0, E)
            return dev.lbs_forward(b.pose, b.trans, shape=b.shape)
        first, n = b.mallocs(call)
        n -= 4                                       # (lbs_forward f64 with shape rows on host buffers: 4)
        assert n == 1                                # the joints' derivative
        live = b.live()
        b.failing(1, lambda: dev.set_free_shape(0, E))
        assert b.live() == live - 1
        for export in (lambda: dev.lbs_forward(b.pose, b.trans, shape=b.shape),
                       lambda: dev.lbs_forward(b.pose, b.trans, shape=b.shape, dtype=np.float32),
                       lambda: dev.posed_joints(b.pose, b.trans, shape=b.shape)):
            with pytest.raises(b.capi.MoshiiError, match='shape coefficients without a block: call moshii_model_set_free_shape first'):
                export()
        assert same(dev.lbs_forward(b.pose, b.trans), frozen)   # the frozen body still exports
        assert same(call(), first) and b.live() == live
    finally:
        dev.close()


FIRST_F32_MALLOCS = 24   # of the first f32 export of a handle with a free shape block: 4 staged buffers (pose, trans, shape, verts), 13 of
                         # moshii_lbs32_prepare (11 arrays of the copy, 2 reduction buffers), 7 grown at the first launch


def _export_f32(b, dev):
    return dev.lbs_forward(b.pose, b.trans, dtype=np.float32, shape=b.shape)


@pytest.fixture(scope='module')
def first_f32(bench):
    """(vertices, hipMalloc calls) of the first f32 export of a fresh handle."""
    dev = bench.model(faces=None)
    try:
        return bench.mallocs(lambda: _export_f32(bench, dev))
    finally:
        dev.close()


def test_first_f32_export_allocation_count(first_f32):
    assert first_f32[1] == FIRST_F32_MALLOCS     # (the cases of the next test are this many)


@pytest.mark.parametrize('nth', range(1, FIRST_F32_MALLOCS + 1))
def test_a_failed_first_f32_export_builds_no_half_copy(bench, first_f32, nth):
    """The first f32 export of a handle stages the call, builds the f32 copy of the model (moshii_lbs32_prepare) and grows the per-call
    scratch: whichever of those allocations fails, all of them are released and the next export is the one of a fresh handle."""
    b = bench
    dev = b.model(faces=None)
    try:
        live = b.live()
        b.failing(nth, lambda: _export_f32(b, dev))
        assert b.live() == live, nth
        assert same(_export_f32(b, dev), first_f32[0]), nth
    finally:
        dev.close()


def test_device_buffer_calls_allocate_nothing(bench):
    """vertex_normals, surface_distance with `face`, joints and the f64 export never allocate on device buffers; virtual_markers,
    marker_surface_distance and the f32 export not from the second call of a size on (the handle keeps their scratch)."""
    b = bench
    capi = b.capi
    dev = b.model()
    keep = []

    def buf(a):
        d = capi.DeviceBuffer(max(a.nbytes, 8))
        d.upload(a)
        keep.append(d)
        return d.ptr

    try:
        for dt in (np.float32, np.float64):
            f32 = dt == np.float32
            v, pts = b.points(dev, dt)
            pose, trans, verts, points = buf(b.pose.astype(dt)), buf(b.trans.astype(dt)), buf(v), buf(pts)
            o = [buf(np.zeros(F * dev.V * 3, dt)) for _ in range(4)]
            never = {
                'vertex_normals': lambda: dev.vertex_normals_device(F, verts, o[0], None, f32=f32),
                'surface_distance': lambda: dev.surface_distance_device(F, verts, N, points, o[0], o[1], o[2], o[3], None, f32=f32),
                'joints': lambda: dev.posed_joints_device(F, pose, trans, o[0], o[1], None, f32=f32),
            }
            if not f32:
                never['lbs_forward_f64'] = lambda: dev.lbs_forward_device(F, pose, trans, o[0], None, f32=False)
            for name, call in never.items():
                assert b.mallocs(call)[1] == 0, (name, dt)
            repeated = {
                'virtual_markers': lambda: dev.virtual_markers_device(F, pose, trans, b.vids, b.dist, o[0], o[1], None, f32=f32),
                'marker_surface_distance': lambda: dev.marker_surface_distance_device(F, pose, trans, N, points, o[0], None, o[2], o[3], None, f32=f32),
                'lbs_forward': lambda: dev.lbs_forward_device(F, pose, trans, o[0], None, f32=f32),
            }
            for name, call in repeated.items():
                call()
                assert b.mallocs(call)[1] == 0, (name, dt)
    finally:
        for d in keep:
            d.close()
        dev.close()
