"""ctypes binding of libmoshii.so (include/moshii.h).

The library is the product: there is NO CPU fallback.  `load()` raises if the shared object is
missing, and every compute entry point returns MOSHII_ERR_NO_DEVICE without a HIP device.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MOSHII_LIB', os.path.join(_HERE, 'libmoshii.so'))
# limits of the chain kernel (include/moshii.h "Limits"): one chain's whole state lives in the 160 KiB LDS of a CU
MAX_MARKERS = 128            # moshii_attach_create
MAX_JOINTS = 64              # moshii_model_create (ancestor sets are 64-bit masks)
MAX_UNKNOWNS = 127           # 3 + free pose variables per solve, plain kernel (8 register blocks of 16, one row for the right-hand side)
MAX_UNKNOWNS_EXTENDED = 207  # ... with the jaw term / a free shape block (13 register blocks)

BUFFERS_HOST = 0
BUFFERS_DEVICE = 1

_c_double_p = C.POINTER(C.c_double)
_c_float_p = C.POINTER(C.c_float)
_c_int_p = C.POINTER(C.c_int32)
_c_u8_p = C.POINTER(C.c_uint8)


class ModelDesc(C.Structure):
    _fields_ = [('V', C.c_int32), ('K', C.c_int32), ('NB', C.c_int32), ('body_dof', C.c_int32),
                ('hand_dof', C.c_int32), ('parents', _c_int_p), ('v_template', _c_double_p),
                ('shapedirs', _c_double_p), ('posedirs', _c_double_p), ('weights', _c_double_p),
                ('J_regressor', _c_double_p), ('hands_mean', _c_double_p), ('selected_components', _c_double_p)]


class SolveOpts(C.Structure):
    _fields_ = [('wt_data', C.c_double), ('wt_velo', C.c_double), ('wt_poseB', C.c_double),
                ('wt_poseH', C.c_double), ('wt_annealing', C.c_double), ('num_train_markers', C.c_double),
                ('e3_first', C.c_double), ('e3', C.c_double), ('delta0', C.c_double), ('maxiter', C.c_int32),
                ('n_step1', C.c_int32), ('step1_ids', _c_int_p), ('n_step2', C.c_int32), ('step2_ids', _c_int_p),
                ('n_body', C.c_int32), ('body_ids', _c_int_p), ('n_finger', C.c_int32), ('finger_ids', _c_int_p),
                ('n_face', C.c_int32), ('face_ids', _c_int_p), ('wt_poseF', C.c_double), ('n_shape', C.c_int32),
                ('wt_shape', C.c_double), ('wt_shape_stay', C.c_double),
                ('n_jangle', C.c_int32), ('jangle_ids', _c_int_p), ('wt_jangle', C.c_double)]


NERR = 8   # MOSHII_NERR: data, poseB, velo, poseH, poseF, shape, shape_stay, poseB_jangles


class ChainDesc(C.Structure):
    _fields_ = [('attach', C.c_void_p), ('F', C.c_int32), ('first_frame_schedule', C.c_int32),
                ('obs', C.c_void_p), ('vis', C.c_void_p), ('init_pose', _c_double_p), ('init_trans', _c_double_p),
                ('init_pose_prev', _c_double_p), ('init_shape', _c_double_p), ('pose', C.c_void_p),
                ('fullpose', C.c_void_p), ('trans', C.c_void_p), ('markers_sim', C.c_void_p), ('errs', C.c_void_p),
                ('iters', C.c_void_p), ('status', C.c_void_p), ('shape', C.c_void_p)]


class SequenceDesc(C.Structure):
    _fields_ = [('attach', C.c_void_p), ('F', C.c_int32), ('obs', C.c_void_p), ('vis', C.c_void_p),
                ('init_pose', _c_double_p), ('init_trans', _c_double_p), ('init_pose_prev', _c_double_p),
                ('pose', C.c_void_p), ('fullpose', C.c_void_p), ('trans', C.c_void_p), ('markers_sim', C.c_void_p),
                ('errs', C.c_void_p), ('iters', C.c_void_p), ('status', C.c_void_p),
                ('init_shape', _c_double_p), ('shape', C.c_void_p)]


class ChunkOpts(C.Structure):
    _fields_ = [('num_chunks', C.c_int32), ('warmup', C.c_int32), ('verify_tol', C.c_double)]


class ChunkReport(C.Structure):
    _fields_ = [('n_chunks', C.c_int32), ('n_repaired', C.c_int32), ('repair_rounds', C.c_int32), ('warmup', C.c_int32),
                ('max_handoff_dev', C.c_double), ('verify_tol', C.c_double)]


class Camera(C.Structure):
    """moshii_camera: X_c = R X_w + t (row major), u = fx X_c.x / X_c.z + cx, v = fy X_c.y / X_c.z + cy; +z forward, y down."""
    _fields_ = [('R', C.c_double * 9), ('t', C.c_double * 3), ('fx', C.c_double), ('fy', C.c_double), ('cx', C.c_double),
                ('cy', C.c_double), ('znear', C.c_double)]

    @classmethod
    def make(cls, R, t, fx, fy, cx, cy, znear):
        c = cls()
        c.R[:] = [float(x) for x in np.asarray(R, dtype=np.float64).reshape(9)]
        c.t[:] = [float(x) for x in np.asarray(t, dtype=np.float64).reshape(3)]
        c.fx, c.fy, c.cx, c.cy, c.znear = float(fx), float(fy), float(cx), float(cy), float(znear)
        return c

    def as_dict(self):
        return dict(R=np.array(self.R[:]).reshape(3, 3), t=np.array(self.t[:]), fx=self.fx, fy=self.fy, cx=self.cx, cy=self.cy,
                    znear=self.znear)


class RenderOpts(C.Structure):
    _fields_ = [('width', C.c_int32), ('height', C.c_int32), ('n_cameras', C.c_int32), ('cameras', C.POINTER(Camera)),
                ('body_rgb', C.c_uint8 * 3), ('bg_rgb', C.c_uint8 * 3), ('ambient', C.c_double), ('point_rgb', _c_u8_p),
                ('point_radius', _c_double_p)]


_P, _I, _U = C.c_void_p, C.c_int32, C.c_uint32
# one argtypes list per f32 / f64 pair of entries: the two differ in what the buffers hold, not in their arguments
_LBS_ARGS = [_P, _I, _P, _P, _P, _U, _P]
_LBS_SHAPE_ARGS = [_P, _I, _P, _P, _P, _P, _U, _P]
_NORMALS_ARGS = [_P, _I, _P, _P, _U, _P]
_VMARKERS_ARGS = [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _U, _P]
_SDIST_ARGS = [_P, _I, _P, _I, _P, _P, _P, _P, _P, _U, _P]
_MSDIST_ARGS = [_P, _I, _P, _P, _P, _I, _P, _P, _P, _P, _P, _U, _P]
_JOINTS_ARGS = [_P, _I, _P, _P, _P, _P, _P, _U, _P]
_RENDER_ARGS = [_P, _I, _P, _I, _P, C.POINTER(RenderOpts), _P, _P, _P, _U, _P]
_RENDER_POSED_ARGS = [_P, _I, _P, _P, _P, _I, _P, C.POINTER(RenderOpts), _P, _P, _P, _U, _P]

EXPORTS = {
    # name: (restype, argtypes)
    'moshii_last_error': (C.c_char_p, []),
    'moshii_version': (C.c_int, []),
    'moshii_source_hash': (C.c_char_p, []),
    'moshii_device_count': (C.c_int, []),
    'moshii_set_device': (C.c_int, [C.c_int]),
    'moshii_device_multiprocessors': (C.c_int, []),
    'moshii_model_create': (C.c_int, [C.POINTER(ModelDesc), C.POINTER(C.c_void_p)]),
    'moshii_model_destroy': (C.c_int, [C.c_void_p]),
    'moshii_model_set_betas': (C.c_int, [C.c_void_p, _c_double_p, C.c_int32]),
    'moshii_model_set_free_shape': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'moshii_model_get_joints': (C.c_int, [C.c_void_p, _c_double_p]),
    'moshii_lbs_forward_f64': (C.c_int, _LBS_ARGS),
    'moshii_lbs_forward_f32': (C.c_int, _LBS_ARGS),
    'moshii_lbs_forward_shape_f64': (C.c_int, _LBS_SHAPE_ARGS),
    'moshii_lbs_forward_shape_f32': (C.c_int, _LBS_SHAPE_ARGS),
    'moshii_model_set_faces': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    'moshii_vertex_normals_f32': (C.c_int, _NORMALS_ARGS),
    'moshii_vertex_normals_f64': (C.c_int, _NORMALS_ARGS),
    'moshii_virtual_markers_f32': (C.c_int, _VMARKERS_ARGS),
    'moshii_virtual_markers_f64': (C.c_int, _VMARKERS_ARGS),
    'moshii_surface_distance_f32': (C.c_int, _SDIST_ARGS),
    'moshii_surface_distance_f64': (C.c_int, _SDIST_ARGS),
    'moshii_marker_surface_distance_f32': (C.c_int, _MSDIST_ARGS),
    'moshii_marker_surface_distance_f64': (C.c_int, _MSDIST_ARGS),
    'moshii_joints_f32': (C.c_int, _JOINTS_ARGS),
    'moshii_joints_f64': (C.c_int, _JOINTS_ARGS),
    'moshii_render_f32': (C.c_int, _RENDER_ARGS),
    'moshii_render_f64': (C.c_int, _RENDER_ARGS),
    'moshii_render_posed_f32': (C.c_int, _RENDER_POSED_ARGS),
    'moshii_render_posed_f64': (C.c_int, _RENDER_POSED_ARGS),
    'moshii_prior_create': (C.c_int, [C.c_int32, C.c_int32, _c_double_p, _c_double_p, _c_double_p, C.POINTER(C.c_void_p)]),
    'moshii_prior_destroy': (C.c_int, [C.c_void_p]),
    'moshii_attach_create': (C.c_int, [C.c_void_p, C.c_int32, _c_int_p, _c_double_p, C.POINTER(C.c_void_p)]),
    'moshii_attach_destroy': (C.c_int, [C.c_void_p]),
    'moshii_attach_markers': (C.c_int, [C.c_void_p, C.c_int32, _c_double_p, _c_double_p, _c_double_p]),
    'moshii_chain_solve': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SolveOpts), C.c_int32, C.POINTER(ChainDesc),
                                     C.c_uint32, C.c_void_p]),
    'moshii_plan_chunks': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _c_int_p, _c_int_p]),
    'moshii_sequence_solve': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(SolveOpts), C.c_int32, C.POINTER(SequenceDesc),
                                        C.POINTER(ChunkOpts), C.c_uint32, C.c_void_p, C.POINTER(ChunkReport)]),
    'moshii_last_launch_info': (C.c_int, [C.c_char_p, C.c_int32, _c_int_p, _c_int_p]),
}

# exported by the library, not part of the C ABI of include/moshii.h: device buffers for DeviceBuffer below
_INTERNAL = {
    'moshii_internal_dev_alloc': (C.c_void_p, [C.c_size_t]),
    'moshii_internal_dev_free': (None, [C.c_void_p]),
    'moshii_internal_dev_copy': (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
}

_lib = None


class MoshiiError(RuntimeError):
    pass


def load():
    """dlopen libmoshii.so (built in-tree by __graft_entry__.build() / moshpp_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MoshiiError(f'{LIB_PATH} not found: build it with `python -m moshpp_amd.build` '
                          f'(there is no CPU fallback for the Stage-II path)')
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(EXPORTS.items()) + list(_INTERNAL.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().moshii_last_error()
        raise MoshiiError(f'libmoshii error {rc}: {msg.decode() if msg else "?"}')


def device_count():
    return load().moshii_device_count()


def device_cu_count():
    """CUs of the current device (256 on MI355X); the default chunk count of the chunked chain modes."""
    return max(int(load().moshii_device_multiprocessors()), 1)


def require_device():
    if device_count() < 1:
        raise MoshiiError('no HIP device visible: the moshpp_amd Stage-II path runs only on the GPU')


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _need_float(who, dtype):
    if dtype not in (np.float64, np.float32):
        raise ValueError(f'{who}: dtype must be numpy float64 or float32, not {dtype!r}')


def _dp(a):
    return a.ctypes.data_as(_c_double_p)


def _ip(a):
    return a.ctypes.data_as(_c_int_p)


class _Owner:
    """Owner of one thing of the library's: close() gives it back once, __del__ does so quietly.  An object that never got as far as
    holding it (a failed or skipped __init__) closes as nothing."""
    _slot, _destroy, _closed = 'handle', None, C.c_void_p   # the attribute, the entry that frees it, what the attribute is afterwards

    def close(self):
        h = getattr(self, self._slot, None)
        if h:
            getattr(load(), self._destroy)(h)
            setattr(self, self._slot, self._closed())

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer(_Owner):
    """A device allocation of the library's own (for callers that chain device-buffer calls without another allocator)."""
    _slot, _destroy, _closed = 'ptr', 'moshii_internal_dev_free', type(None)

    def __init__(self, nbytes):
        lib = load()
        self.nbytes = int(nbytes)
        self.ptr = lib.moshii_internal_dev_alloc(self.nbytes)
        if not self.ptr:
            raise MoshiiError(f'device allocation of {self.nbytes} bytes failed')

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        if load().moshii_internal_dev_copy(self.ptr, a.ctypes.data, a.nbytes, 1):
            raise MoshiiError('host -> device copy failed')

    def download(self, out):
        assert out.flags.c_contiguous and out.nbytes <= self.nbytes
        if load().moshii_internal_dev_copy(out.ctypes.data, self.ptr, out.nbytes, 0):
            raise MoshiiError('device -> host copy failed')
        return out


class SurfaceDistance:
    """What Model.surface_distance / marker_surface_distance return: distance[F, N] (signed, metres), face[F, N], part[F, N]
    (0 interior, 1-3 edges ab / bc / ca, 4-6 vertices a / b / c; -1 for an absent point), nearest[F, N, 3]."""
    __slots__ = ('distance', 'face', 'part', 'nearest')

    def __init__(self, distance, face, part, nearest):
        self.distance, self.face, self.part, self.nearest = distance, face, part, nearest

    @classmethod
    def empty(cls, F, N, dtype):
        return cls(np.zeros((F, N), dtype=dtype), np.zeros((F, N), dtype=np.int32), np.zeros((F, N), dtype=np.int32),
                   np.zeros((F, N, 3), dtype=dtype))


class Model(_Owner):
    """moshii_model_t: body model arrays + pose-variable layout, resident in HBM."""
    _destroy = 'moshii_model_destroy'

    def __init__(self, v_template, shapedirs, posedirs, weights, J_regressor, parents, body_dof, hand_dof=0,
                 hands_mean=None, selected_components=None):
        lib = load()
        require_device()
        v_template = _f64(v_template)
        V = v_template.shape[0]
        parents = np.ascontiguousarray(parents, dtype=np.int32)
        K = parents.shape[0]
        shapedirs = _f64(shapedirs)
        if hasattr(J_regressor, 'toarray'):
            J_regressor = J_regressor.toarray()
        J_regressor = _f64(J_regressor)
        posedirs = _f64(posedirs)
        posedirs = posedirs.reshape(V, 3, posedirs.size // max(3 * V, 1))   # (a one-joint model has no pose features: zero columns)
        weights = _f64(weights)
        assert posedirs.shape[2] == 9 * (K - 1), (posedirs.shape, K)
        assert weights.shape == (V, K) and J_regressor.shape == (K, V)
        NB = shapedirs.shape[-1]
        d = ModelDesc()
        d.V, d.K, d.NB, d.body_dof, d.hand_dof = V, K, NB, int(body_dof), int(hand_dof)
        keep = [parents, v_template, shapedirs, posedirs, weights, J_regressor]
        d.parents = _ip(parents)
        d.v_template = _dp(v_template); d.shapedirs = _dp(shapedirs); d.posedirs = _dp(posedirs)
        d.weights = _dp(weights); d.J_regressor = _dp(J_regressor)
        if hand_dof:
            hm = _f64(hands_mean); sc = _f64(selected_components)
            assert hm.shape == (3 * K - body_dof,) and sc.shape == (hand_dof, 3 * K - body_dof)
            keep += [hm, sc]
            d.hands_mean = _dp(hm); d.selected_components = _dp(sc)
        self.V, self.K, self.NB, self.body_dof, self.hand_dof = V, K, NB, int(body_dof), int(hand_dof)
        self.P = 3 * K
        self.NP = self.body_dof + self.hand_dof
        self.handle = C.c_void_p()
        check(lib.moshii_model_create(C.byref(d), C.byref(self.handle)))
        del keep

    def set_betas(self, betas):
        b = _f64(np.ravel(betas))
        check(load().moshii_model_set_betas(self.handle, _dp(b), b.shape[0]))

    def set_free_shape(self, start, count):
        """Shapedirs columns [start, start+count) become Step-2 free variables (expression / DMPL); call before
        creating attachments."""
        check(load().moshii_model_set_free_shape(self.handle, int(start), int(count)))
        self.n_free_shape = int(count)

    def joints(self):
        out = np.zeros((self.K, 3))
        check(load().moshii_model_get_joints(self.handle, _dp(out)))
        return out

    def lbs_forward(self, pose, trans, dtype=np.float64, shape=None):
        """verts[F,V,3] for pose variables pose[F,NP], trans[F,3] (host arrays).  shape[F, nshape]: per-frame coefficients of the
        block declared with set_free_shape (the `shape` a Stage-II solve returns: expression / DMPL offsets on the frozen betas);
        rest positions and joints follow them."""
        _need_float('lbs_forward', dtype)
        pose, trans, shape, F = self._posed_inputs('lbs_forward', pose, trans, shape, dtype)
        out = np.zeros((F, self.V, 3), dtype=dtype)
        if shape is None:
            fn = self._entry('lbs_forward', dtype == np.float32)
            check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, out.ctypes.data, BUFFERS_HOST, None))
        else:
            fn = self._entry('lbs_forward_shape', dtype == np.float32)
            check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, shape.ctypes.data, out.ctypes.data, BUFFERS_HOST, None))
        return out

    @staticmethod
    def _entry(stem, f32):
        """The library's moshii_<stem>_f32 or moshii_<stem>_f64."""
        return getattr(load(), 'moshii_' + stem + ('_f32' if f32 else '_f64'))

    def _posed_inputs(self, who, pose, trans, shape, dtype):
        """(pose[F, NP], trans[F, 3], shape[F, nshape] | None, F) as contiguous arrays of `dtype` (checked by the caller, _need_float, ahead
        of its own checks); ValueError, before any device call, if they cannot be that."""
        pose = np.ascontiguousarray(np.atleast_2d(pose), dtype=dtype)
        trans = np.ascontiguousarray(np.atleast_2d(trans), dtype=dtype)
        F = pose.shape[0]
        if pose.shape != (F, self.NP) or trans.shape != (F, 3):
            raise ValueError(f'{who}: pose / trans must be [F, {self.NP}] / [F, 3], got {pose.shape} / {trans.shape}')
        if shape is not None:
            shape = self._check_shape_rows(shape, F, dtype)
        return pose, trans, shape, F

    def _mesh_inputs(self, who, verts, dtype=None):
        """verts[F, V, 3] (a lone [V, 3] becomes [1, V, 3]) as a contiguous array of `dtype`; None: of its own dtype, which must then be
        float32 or float64."""
        verts = np.asarray(verts)
        if dtype is None and verts.dtype not in (np.float32, np.float64):
            raise ValueError(f'{who}: verts must be float32 or float64, not {verts.dtype}')
        v = verts[None] if verts.ndim == 2 else verts
        if v.ndim != 3 or v.shape[1:] != (self.V, 3):
            raise ValueError(f'{who}: verts must be [F, {self.V}, 3], got {tuple(verts.shape)}')
        return np.ascontiguousarray(v, dtype=dtype)

    def _check_shape_rows(self, shape, F, dtype):
        """shape[F, nshape] as a contiguous array of `dtype`; ValueError (before any device call) if it cannot be that."""
        n = int(getattr(self, 'n_free_shape', 0))
        if n <= 0:
            raise ValueError('lbs_forward: shape coefficients given, but the model has no free shape block (set_free_shape)')
        shape = np.asarray(shape)
        if shape.ndim == 1 and F == 1:
            shape = shape[None]
        if shape.ndim != 2 or shape.shape != (F, n):
            raise ValueError(f'lbs_forward: shape must be [F, nshape] = [{F}, {n}], got {tuple(shape.shape)}')
        if not np.issubdtype(shape.dtype, np.number) or np.iscomplexobj(shape):
            raise ValueError(f'lbs_forward: shape must be real numbers, got dtype {shape.dtype}')
        shape = np.ascontiguousarray(shape, dtype=dtype)
        if not np.isfinite(shape).all():
            raise ValueError('lbs_forward: shape holds non-finite coefficients')
        return shape

    # ---- the mesh as a surface: faces, vertex normals, virtual markers ----
    def set_faces(self, faces):
        """Triangles faces[n, 3] (vertex ids) for vertex_normals / virtual_markers; an empty list clears them."""
        faces = np.asarray(faces)
        if faces.size == 0:
            faces = np.zeros((0, 3), dtype=np.int32)
        if faces.ndim != 2 or faces.shape[1] != 3 or not np.issubdtype(faces.dtype, np.integer):
            raise ValueError(f'set_faces: faces must be integers [n, 3], got {faces.dtype} {tuple(faces.shape)}')
        if len(faces) and (faces.min() < 0 or faces.max() >= self.V):
            raise ValueError(f'set_faces: vertex ids outside [0, {self.V})')
        faces = np.ascontiguousarray(faces, dtype=np.int32)
        check(load().moshii_model_set_faces(self.handle, len(faces), faces.ctypes.data if len(faces) else None))
        self.n_faces = len(faces)

    def _need_faces(self, who):
        if int(getattr(self, 'n_faces', 0)) <= 0:
            raise ValueError(f'{who}: the model has no faces (set_faces)')

    def _need_free_shape(self, who, shape_ptr):
        if shape_ptr is not None and int(getattr(self, 'n_free_shape', 0)) <= 0:
            raise ValueError(f'{who}: shape_ptr given, but the model has no free shape block (set_free_shape)')

    def vertex_normals(self, verts):
        """Area-weighted unit vertex normals [F, V, 3] of the meshes verts[F, V, 3] (or [V, 3]); float32 or float64 as the array."""
        self._need_faces('vertex_normals')
        verts = np.asarray(verts)
        v = self._mesh_inputs('vertex_normals', verts)
        out = np.zeros_like(v)
        fn = self._entry('vertex_normals', v.dtype == np.float32)
        check(fn(self.handle, v.shape[0], v.ctypes.data, out.ctypes.data, BUFFERS_HOST, None))
        return out[0] if verts.ndim == 2 else out

    def vertex_normals_device(self, F, verts_ptr, normals_ptr, stream=None, f32=True):
        self._need_faces('vertex_normals_device')
        fn = self._entry('vertex_normals', f32)
        check(fn(self.handle, F, verts_ptr, normals_ptr, BUFFERS_DEVICE, stream))

    def _check_markers(self, vids, dist, dtype, who):
        vids = np.asarray(vids)
        if vids.ndim != 1 or len(vids) < 1 or not np.issubdtype(vids.dtype, np.integer):
            raise ValueError(f'{who}: vids must be a non-empty list of integer vertex ids')
        if vids.min() < 0 or vids.max() >= self.V:
            raise ValueError(f'{who}: vids outside [0, {self.V})')
        dist = np.asarray(dist, dtype=np.float64)
        if dist.ndim == 0:
            dist = np.full(len(vids), float(dist))
        if dist.shape != vids.shape or not np.isfinite(dist).all():
            raise ValueError(f'{who}: dist must be {len(vids)} finite distances (metres)')
        return np.ascontiguousarray(vids, dtype=np.int32), np.ascontiguousarray(dist, dtype=dtype)

    def virtual_markers(self, pose, trans, vids, dist, dtype=np.float64, shape=None, return_normals=False):
        """markers[F, M, 3] = verts_f[vids] + dist * vertex normal, frame by frame, for pose variables pose[F, NP], trans[F, 3] (host
        arrays) -- the meshes never leave the device.  shape as in lbs_forward.  return_normals: (markers, normals[F, M, 3])."""
        _need_float('virtual_markers', dtype)
        self._need_faces('virtual_markers')
        vids, dist = self._check_markers(vids, dist, dtype, 'virtual_markers')
        pose, trans, shape, F = self._posed_inputs('virtual_markers', pose, trans, shape, dtype)
        M = len(vids)
        out = np.zeros((F, M, 3), dtype=dtype)
        nrm = np.zeros((F, M, 3), dtype=dtype) if return_normals else None
        fn = self._entry('virtual_markers', dtype == np.float32)
        check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, shape.ctypes.data if shape is not None else None, M,
                 vids.ctypes.data, dist.ctypes.data, out.ctypes.data, nrm.ctypes.data if return_normals else None, BUFFERS_HOST, None))
        return (out, nrm) if return_normals else out

    def virtual_markers_device(self, F, pose_ptr, trans_ptr, vids, dist, out_ptr, normals_ptr=None, stream=None, f32=True, shape_ptr=None):
        """Device buffers for pose / trans / shape / markers / normals; vids and dist are host arrays."""
        self._need_faces('virtual_markers_device')
        vids, dist = self._check_markers(vids, dist, np.float32 if f32 else np.float64, 'virtual_markers_device')
        fn = self._entry('virtual_markers', f32)
        check(fn(self.handle, F, pose_ptr, trans_ptr, shape_ptr, len(vids), vids.ctypes.data, dist.ctypes.data, out_ptr, normals_ptr,
                 BUFFERS_DEVICE, stream))

    # ---- signed point-to-mesh distance ----
    def _check_points(self, points, F, dtype, who):
        """points[F, N, 3] (or [N, 3] with F == 1) as a contiguous array of `dtype`; NaN rows are absent points."""
        points = np.asarray(points)
        if points.ndim == 2 and F == 1:
            points = points[None]
        if points.ndim != 3 or points.shape[0] != F or points.shape[2] != 3:
            raise ValueError(f'{who}: points must be [F, N, 3] = [{F}, N, 3], got {tuple(points.shape)}')
        if not np.issubdtype(points.dtype, np.number) or np.iscomplexobj(points):
            raise ValueError(f'{who}: points must be real numbers, got dtype {points.dtype}')
        return np.ascontiguousarray(points, dtype=dtype)

    def surface_distance(self, verts, points, dtype=None):
        """Signed distance (metres, positive outside) of points[F, N, 3] to the meshes verts[F, V, 3] with the model's faces:
        SurfaceDistance(distance[F, N], face[F, N], part[F, N], nearest[F, N, 3]).  dtype: numpy float32 or float64 (default: that of
        verts).  A point with a NaN coordinate is absent: distance NaN, face -1, part -1, nearest NaN."""
        verts = np.asarray(verts)
        if dtype is None:
            dtype = np.float32 if verts.dtype == np.float32 else np.float64
        _need_float('surface_distance', dtype)
        self._need_faces('surface_distance')
        v = self._mesh_inputs('surface_distance', verts, dtype)
        F = v.shape[0]
        points = self._check_points(points, F, dtype, 'surface_distance')
        res = SurfaceDistance.empty(F, points.shape[1], dtype)
        fn = self._entry('surface_distance', dtype == np.float32)
        check(fn(self.handle, F, v.ctypes.data, points.shape[1], points.ctypes.data, res.distance.ctypes.data, res.face.ctypes.data,
                 res.part.ctypes.data, res.nearest.ctypes.data, BUFFERS_HOST, None))
        return res

    def surface_distance_device(self, F, verts_ptr, N, points_ptr, dist_ptr, face_ptr=None, part_ptr=None, nearest_ptr=None, stream=None,
                                f32=True):
        """Device buffers (f32: float, else double; face / part int32); asynchronous on `stream`."""
        self._need_faces('surface_distance_device')
        fn = self._entry('surface_distance', f32)
        check(fn(self.handle, F, verts_ptr, N, points_ptr, dist_ptr, face_ptr, part_ptr, nearest_ptr, BUFFERS_DEVICE, stream))

    def marker_surface_distance(self, pose, trans, points, shape=None, dtype=np.float64):
        """surface_distance of points[F, N, 3] against the meshes of pose[F, NP], trans[F, 3] (shape as in lbs_forward) -- the meshes
        never leave the device."""
        _need_float('marker_surface_distance', dtype)
        self._need_faces('marker_surface_distance')
        pose, trans, shape, F = self._posed_inputs('marker_surface_distance', pose, trans, shape, dtype)
        points = self._check_points(points, F, dtype, 'marker_surface_distance')
        res = SurfaceDistance.empty(F, points.shape[1], dtype)
        fn = self._entry('marker_surface_distance', dtype == np.float32)
        check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, shape.ctypes.data if shape is not None else None, points.shape[1],
                 points.ctypes.data, res.distance.ctypes.data, res.face.ctypes.data, res.part.ctypes.data, res.nearest.ctypes.data,
                 BUFFERS_HOST, None))
        return res

    def marker_surface_distance_device(self, F, pose_ptr, trans_ptr, N, points_ptr, dist_ptr, face_ptr=None, part_ptr=None, nearest_ptr=None,
                                       stream=None, f32=True, shape_ptr=None):
        """Device buffers for pose / trans / shape / points and the results; asynchronous on `stream`."""
        self._need_faces('marker_surface_distance_device')
        self._need_free_shape('marker_surface_distance_device', shape_ptr)
        fn = self._entry('marker_surface_distance', f32)
        check(fn(self.handle, F, pose_ptr, trans_ptr, shape_ptr, N, points_ptr, dist_ptr, face_ptr, part_ptr, nearest_ptr, BUFFERS_DEVICE, stream))

    # ---- the skeleton: posed joints and world joint rotations ----
    def posed_joints(self, pose, trans, shape=None, dtype=np.float64, return_rotations=False):
        """joints[F, K, 3]: the world position of every joint (translation included) for pose variables pose[F, NP], trans[F, 3] (host
        arrays) -- forward kinematics alone, the reference's J_transformed.  shape as in lbs_forward (the joints move with the
        coefficients).  return_rotations: (joints, rot[F, K, 3, 3]), the world rotation of every joint (A_global's rotation part).
        float32 computes in float64 and rounds once.  joints() stays the REST joints."""
        _need_float('posed_joints', dtype)
        pose, trans, shape, F = self._posed_inputs('posed_joints', pose, trans, shape, dtype)
        out = np.zeros((F, self.K, 3), dtype=dtype)
        rot = np.zeros((F, self.K, 3, 3), dtype=dtype) if return_rotations else None
        fn = self._entry('joints', dtype == np.float32)
        check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, shape.ctypes.data if shape is not None else None, out.ctypes.data,
                 rot.ctypes.data if return_rotations else None, BUFFERS_HOST, None))
        return (out, rot) if return_rotations else out

    def posed_joints_device(self, F, pose_ptr, trans_ptr, out_ptr, rot_ptr=None, stream=None, f32=True, shape_ptr=None):
        """Device buffers (f32: float, else double) for pose / trans / shape / joints[F][K][3] / rot[F][K][3][3]; asynchronous on
        `stream`."""
        self._need_free_shape('posed_joints_device', shape_ptr)
        fn = self._entry('joints', f32)
        check(fn(self.handle, F, pose_ptr, trans_ptr, shape_ptr, out_ptr, rot_ptr, BUFFERS_DEVICE, stream))

    # ---- shaded previews ----
    def _render_opts(self, who, F, cameras, size, N, point_rgb, point_radius, body_rgb, bg_rgb, ambient):
        """(RenderOpts, objects it points to) for F frames and N points; ValueError on what the library would refuse."""
        try:
            W, H = (int(x) for x in size)
        except (TypeError, ValueError):
            raise ValueError(f'{who}: size must be (width, height), got {size!r}')
        if not (1 <= W <= 4096 and 1 <= H <= 4096):
            raise ValueError(f'{who}: width and height must be within 1 .. 4096, got {W} x {H}')
        if isinstance(cameras, Camera):
            cameras = [cameras]
        cameras = list(cameras)
        if not all(isinstance(c, Camera) for c in cameras):
            raise ValueError(f'{who}: cameras must be capi.Camera objects')
        if len(cameras) != 1 and len(cameras) != F:
            raise ValueError(f'{who}: one camera or one per frame ({F}), got {len(cameras)}')
        if not 0.0 <= float(ambient) <= 1.0:
            raise ValueError(f'{who}: ambient must be within 0 .. 1, got {ambient}')
        o = RenderOpts()
        cams = (Camera * len(cameras))(*cameras)
        o.width, o.height, o.n_cameras, o.cameras = W, H, len(cameras), cams
        o.body_rgb[:] = [int(x) for x in np.asarray(body_rgb, dtype=np.uint8).reshape(3)]
        o.bg_rgb[:] = [int(x) for x in np.asarray(bg_rgb, dtype=np.uint8).reshape(3)]
        o.ambient = float(ambient)
        keep = [cams]
        if N > 0:
            if point_rgb is None or point_radius is None:
                raise ValueError(f'{who}: points need point_rgb and point_radius')
            prgb = np.asarray(point_rgb, dtype=np.uint8)
            prgb = np.ascontiguousarray(np.broadcast_to(prgb, (N, 3)))
            prad = np.asarray(point_radius, dtype=np.float64)
            prad = np.ascontiguousarray(np.broadcast_to(prad, (N,)))
            o.point_rgb = prgb.ctypes.data_as(_c_u8_p); o.point_radius = _dp(prad)
            keep += [prgb, prad]
        return o, keep

    @staticmethod
    def _render_outputs(F, W, H, outputs):
        bad = set(outputs) - {'rgb', 'ids', 'depth'}
        if bad or not outputs:
            raise ValueError(f"render: outputs must name some of 'rgb', 'ids', 'depth', got {tuple(outputs)!r}")
        res = {}
        if 'rgb' in outputs:
            res['rgb'] = np.zeros((F, H, W, 3), dtype=np.uint8)
        if 'ids' in outputs:
            res['ids'] = np.zeros((F, H, W), dtype=np.int32)
        if 'depth' in outputs:
            res['depth'] = np.zeros((F, H, W), dtype=np.float32)
        return res

    def render(self, verts, cameras, size, points=None, point_rgb=None, point_radius=None, body_rgb=(200, 170, 150), bg_rgb=(255, 255, 255),
               ambient=0.3, outputs=('rgb', 'ids', 'depth')):
        """Shaded previews of the meshes verts[F, V, 3] (float32 or float64, host) with the model's faces, by the rendering rules of
        include/moshii.h: dict(rgb[F, H, W, 3] uint8, ids[F, H, W] int32, depth[F, H, W] float32) of the `outputs` asked for.
        cameras: one capi.Camera or one per frame; size = (width, height); points[F, N, 3] with point_rgb[N, 3] (or one colour) and
        point_radius[N] (or one radius, metres) are drawn as shaded discs, a NaN point is skipped.  ids: face id, n_faces + k for point
        k, -1 for background (depth +inf)."""
        self._need_faces('render')
        v = self._mesh_inputs('render', verts)
        F = v.shape[0]
        N = 0
        if points is not None:
            points = self._check_points(points, F, v.dtype, 'render')
            N = points.shape[1]
        o, keep = self._render_opts('render', F, cameras, size, N, point_rgb, point_radius, body_rgb, bg_rgb, ambient)
        res = self._render_outputs(F, o.width, o.height, outputs)
        fn = self._entry('render', v.dtype == np.float32)
        check(fn(self.handle, F, v.ctypes.data, N, points.ctypes.data if N else None, C.byref(o),
                 *(res[k].ctypes.data if k in res else None for k in ('rgb', 'ids', 'depth')), BUFFERS_HOST, None))
        del keep
        return res

    def render_posed(self, pose, trans, cameras, size, points=None, point_rgb=None, point_radius=None, shape=None, dtype=np.float32,
                     body_rgb=(200, 170, 150), bg_rgb=(255, 255, 255), ambient=0.3, outputs=('rgb', 'ids', 'depth')):
        """render() of the meshes of pose[F, NP], trans[F, 3] (shape as in lbs_forward) -- the meshes never leave the device."""
        _need_float('render_posed', dtype)
        self._need_faces('render_posed')
        pose, trans, shape, F = self._posed_inputs('render_posed', pose, trans, shape, dtype)
        N = 0
        if points is not None:
            points = self._check_points(points, F, dtype, 'render_posed')
            N = points.shape[1]
        o, keep = self._render_opts('render_posed', F, cameras, size, N, point_rgb, point_radius, body_rgb, bg_rgb, ambient)
        res = self._render_outputs(F, o.width, o.height, outputs)
        fn = self._entry('render_posed', dtype == np.float32)
        check(fn(self.handle, F, pose.ctypes.data, trans.ctypes.data, shape.ctypes.data if shape is not None else None, N,
                 points.ctypes.data if N else None, C.byref(o), *(res[k].ctypes.data if k in res else None for k in ('rgb', 'ids', 'depth')),
                 BUFFERS_HOST, None))
        del keep
        return res

    def render_device(self, F, verts_ptr, cameras, size, N=0, points_ptr=None, point_rgb=None, point_radius=None, rgb_ptr=None, ids_ptr=None,
                      depth_ptr=None, body_rgb=(200, 170, 150), bg_rgb=(255, 255, 255), ambient=0.3, stream=None, f32=True):
        """Device buffers for verts / points / rgb / ids / depth; cameras, colours and radii are host data; asynchronous on `stream`."""
        self._need_faces('render_device')
        o, keep = self._render_opts('render_device', F, cameras, size, N, point_rgb, point_radius, body_rgb, bg_rgb, ambient)
        fn = self._entry('render', f32)
        check(fn(self.handle, F, verts_ptr, N, points_ptr, C.byref(o), rgb_ptr, ids_ptr, depth_ptr, BUFFERS_DEVICE, stream))
        del keep

    def render_posed_device(self, F, pose_ptr, trans_ptr, cameras, size, N=0, points_ptr=None, point_rgb=None, point_radius=None, rgb_ptr=None,
                            ids_ptr=None, depth_ptr=None, body_rgb=(200, 170, 150), bg_rgb=(255, 255, 255), ambient=0.3, stream=None, f32=True,
                            shape_ptr=None):
        """Device buffers for pose / trans / shape / points and the outputs; asynchronous on `stream`."""
        self._need_faces('render_posed_device')
        self._need_free_shape('render_posed_device', shape_ptr)
        o, keep = self._render_opts('render_posed_device', F, cameras, size, N, point_rgb, point_radius, body_rgb, bg_rgb, ambient)
        fn = self._entry('render_posed', f32)
        check(fn(self.handle, F, pose_ptr, trans_ptr, shape_ptr, N, points_ptr, C.byref(o), rgb_ptr, ids_ptr, depth_ptr, BUFFERS_DEVICE, stream))
        del keep

    def lbs_forward_with_normals(self, pose, trans, dtype=np.float32, shape=None):
        """(verts, normals), both [F, V, 3]: the export into a device buffer, the normals from that buffer, two copies back -- the
        vertices do not visit the host in between."""
        _need_float('lbs_forward_with_normals', dtype)
        self._need_faces('lbs_forward_with_normals')
        pose, trans, shape, F = self._posed_inputs('lbs_forward_with_normals', pose, trans, shape, dtype)
        verts = np.zeros((F, self.V, 3), dtype=dtype)
        normals = np.zeros_like(verts)
        if F == 0:
            return verts, normals
        bufs = [DeviceBuffer(a.nbytes) for a in (pose, trans, verts, normals)] + ([DeviceBuffer(shape.nbytes)] if shape is not None else [])
        try:
            bufs[0].upload(pose); bufs[1].upload(trans)
            if shape is not None:
                bufs[4].upload(shape)
            f32 = dtype == np.float32
            self.lbs_forward_device(F, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, f32=f32, shape_ptr=bufs[4].ptr if shape is not None else None)
            self.vertex_normals_device(F, bufs[2].ptr, bufs[3].ptr, None, f32=f32)
            bufs[2].download(verts); bufs[3].download(normals)      # (blocking copies on the null stream: behind both kernels)
        finally:
            for b in bufs:
                b.close()
        return verts, normals

    def lbs_forward_device(self, F, pose_ptr, trans_ptr, out_ptr, stream=None, f32=True, shape_ptr=None):
        """Device buffers (f32: float, else double).  shape_ptr: [F][nshape] coefficients of the free shape block on the device."""
        if shape_ptr is None:
            fn = self._entry('lbs_forward', f32)
            check(fn(self.handle, F, pose_ptr, trans_ptr, out_ptr, BUFFERS_DEVICE, stream))
        else:
            self._need_free_shape('lbs_forward_device', shape_ptr)
            fn = self._entry('lbs_forward_shape', f32)
            check(fn(self.handle, F, pose_ptr, trans_ptr, shape_ptr, out_ptr, BUFFERS_DEVICE, stream))



class Prior(_Owner):
    """moshii_prior_t: prepared max-mixture prior (means, chols of precisions, re-normalised weights)."""
    _destroy = 'moshii_prior_destroy'

    def __init__(self, means, chols, weights):
        means = _f64(means); chols = _f64(chols); weights = _f64(np.ravel(weights))
        G, npose = means.shape
        assert chols.shape == (G, npose, npose) and weights.shape == (G,)
        self.G, self.npose = G, npose
        self.handle = C.c_void_p()
        check(load().moshii_prior_create(G, npose, _dp(means), _dp(chols), _dp(weights), C.byref(self.handle)))



class Attachment(_Owner):
    """moshii_attach_t: closest[M,3] vertex ids + coef[M,3] -> compact marker-vertex model slice."""
    _destroy = 'moshii_attach_destroy'

    def __init__(self, model: Model, closest, coef):
        closest = np.ascontiguousarray(closest, dtype=np.int32)
        coef = _f64(coef)
        M = closest.shape[0]
        assert closest.shape == (M, 3) and coef.shape == (M, 3)
        self.model = model
        self.M = M
        self.handle = C.c_void_p()
        check(load().moshii_attach_create(model.handle, M, _ip(closest), _dp(coef), C.byref(self.handle)))

    def markers(self, pose, trans):
        pose = _f64(np.atleast_2d(pose)); trans = _f64(np.atleast_2d(trans))
        F = pose.shape[0]
        out = np.zeros((F, self.M, 3))
        check(load().moshii_attach_markers(self.handle, F, _dp(pose), _dp(trans), _dp(out)))
        return out



def make_opts(weights, step1_ids, step2_ids, body_ids, finger_ids, maxiter=100, e3_first=1e-3, e3=1e-2,
              delta0=0.5, num_train_markers=46.0, face_ids=(), n_shape=0, shape_kind=None, jangle_ids=(), wt_jangle=2.0):
    """SolveOpts + the arrays it points to (keep the returned tuple alive during the call).
    face_ids: jaw pose ids of optimize_face (also part of step2_ids); n_shape / shape_kind ('expr' | 'dmpl'): the free
    shape block declared with Model.set_free_shape.  jangle_ids: the pose ids of the SMAL horse's joint-angle term
    (chmosh.STAGEII_JANGLE_IDS), weighted wt_pose * wt_jangle; empty: no such term."""
    o = SolveOpts()
    o.wt_data = float(weights['stageii_wt_data']); o.wt_velo = float(weights['stageii_wt_velo'])
    o.wt_poseB = float(weights['stageii_wt_poseB']); o.wt_poseH = float(weights['stageii_wt_poseH'])
    o.wt_annealing = float(weights['stageii_wt_annealing'])
    o.num_train_markers = float(num_train_markers)
    o.e3_first, o.e3, o.delta0, o.maxiter = float(e3_first), float(e3), float(delta0), int(maxiter)
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (step1_ids, step2_ids, body_ids, finger_ids, face_ids)]
    o.n_step1, o.n_step2, o.n_body, o.n_finger, o.n_face = (len(a) for a in arrs)
    o.step1_ids, o.step2_ids, o.body_ids, o.finger_ids, o.face_ids = (_ip(a) for a in arrs)
    o.wt_poseF = float(weights.get('stageii_wt_poseF', 1.0))
    o.n_shape = int(n_shape)
    if o.n_shape:
        assert shape_kind in ('expr', 'dmpl')
        o.wt_shape = float(weights['stageii_wt_expr' if shape_kind == 'expr' else 'stageii_wt_dmpl'])
        o.wt_shape_stay = 6.0 if shape_kind == 'dmpl' else 0.0     # chmosh.py:697
    if len(jangle_ids):
        ja = np.ascontiguousarray(jangle_ids, dtype=np.int32)
        arrs.append(ja)
        o.n_jangle, o.jangle_ids, o.wt_jangle = len(ja), _ip(ja), float(wt_jangle)
    return o, arrs


def coop_group(g):
    """MOSHII_COOP_GROUP(g) of include/moshii.h: the cooperative-chain request in the `flags` of moshii_chain_solve."""
    return (int(g) & 0xff) << 8


def chain_solve_host(model: Model, prior, opts_tuple, chains, coop=0):
    """Run moshii_chain_solve on host buffers.
    chains: list of dict(attach, obs[F,M,3], vis[F,M], first=True, init_pose=None, init_trans=None, init_pose_prev=None,
    init_shape=None).  Returns list of dict(pose, fullpose, trans, markers_sim, errs[F,NERR], iters, status, shape[F,n_shape]).
    coop = g > 0: cooperative chains, g workgroups (CUs) per chain (MOSHII_COOP_GROUP(g) in the flags of the C ABI)."""
    lib = load()
    opts, _keep = opts_tuple
    n = len(chains)
    descs = (ChainDesc * n)()
    outs, keep = [], []
    for i, ch in enumerate(chains):
        att = ch['attach']
        obs = _f64(ch['obs']); vis = np.ascontiguousarray(ch['vis'], dtype=np.uint8)
        F, M = vis.shape
        assert obs.shape == (F, M, 3) and M == att.M
        o = dict(pose=np.zeros((F, model.NP)), fullpose=np.zeros((F, model.P)), trans=np.zeros((F, 3)),
                 markers_sim=np.zeros((F, M, 3)), errs=np.zeros((F, NERR)), iters=np.zeros((F, 2), dtype=np.int32),
                 status=np.zeros(F, dtype=np.int32), shape=np.zeros((F, int(opts.n_shape))))
        d = descs[i]
        d.attach = att.handle
        d.F = F
        d.first_frame_schedule = 1 if ch.get('first', True) else 0
        d.obs = obs.ctypes.data
        d.vis = vis.ctypes.data
        keep += [obs, vis]
        for key, fld in (('init_pose', 'init_pose'), ('init_trans', 'init_trans'), ('init_pose_prev', 'init_pose_prev'),
                         ('init_shape', 'init_shape')):
            if ch.get(key) is not None:
                a = _f64(ch[key]); keep.append(a)
                setattr(d, fld, _dp(a))
        for key in ('pose', 'fullpose', 'trans', 'markers_sim', 'errs', 'iters', 'status'):
            setattr(d, key, o[key].ctypes.data)
        if opts.n_shape:
            d.shape = o['shape'].ctypes.data
        outs.append(o)
    check(lib.moshii_chain_solve(model.handle, prior.handle if prior is not None else None, C.byref(opts), n, descs,
                                 BUFFERS_HOST | coop_group(coop), None))
    del keep
    return outs


def plan_chunks(F, num_chunks, warmup, cap=1 << 20):
    """moshii_plan_chunks -> (starts, launch_starts) int32 arrays (host arithmetic only; works without a GPU)."""
    n = max(1, int(num_chunks))
    starts = np.zeros(n, dtype=np.int32); launch = np.zeros(n, dtype=np.int32)
    c = load().moshii_plan_chunks(int(F), n, int(warmup), int(cap), _ip(starts), _ip(launch))
    if c < 0:
        check(c)
    return starts[:c].copy(), launch[:c].copy()


def sequence_solve_host(model: Model, prior, opts_tuple, seqs, num_chunks=0, warmup=32, verify_tol=1e-11, coop=0):
    """moshii_sequence_solve on host buffers.  seqs: list of dict(attach, obs[F,M,3], vis[F,M], init_pose=None,
    init_trans=None, init_pose_prev=None) -- with init_* the sequence continues a chain from that state instead of running
    the first-frame schedule.  Returns (list of per-sequence output dicts as chain_solve_host, report dict)."""
    lib = load()
    opts, _keep = opts_tuple
    n = len(seqs)
    descs = (SequenceDesc * n)()
    outs, keep = [], []
    for i, sq in enumerate(seqs):
        att = sq['attach']
        obs = _f64(sq['obs']); vis = np.ascontiguousarray(sq['vis'], dtype=np.uint8)
        F, M = vis.shape
        assert obs.shape == (F, M, 3) and M == att.M
        o = dict(pose=np.zeros((F, model.NP)), fullpose=np.zeros((F, model.P)), trans=np.zeros((F, 3)),
                 markers_sim=np.zeros((F, M, 3)), errs=np.zeros((F, NERR)), iters=np.zeros((F, 2), dtype=np.int32),
                 status=np.zeros(F, dtype=np.int32), shape=np.zeros((F, int(opts.n_shape))))
        d = descs[i]
        d.attach = att.handle; d.F = F; d.obs = obs.ctypes.data; d.vis = vis.ctypes.data
        keep += [obs, vis]
        for key in ('init_pose', 'init_trans', 'init_pose_prev', 'init_shape'):
            if sq.get(key) is not None:
                a = _f64(sq[key]); keep.append(a)
                setattr(d, key, _dp(a))
        for key in ('pose', 'fullpose', 'trans', 'markers_sim', 'errs', 'iters', 'status'):
            setattr(d, key, o[key].ctypes.data)
        if int(opts.n_shape):
            d.shape = o['shape'].ctypes.data
        outs.append(o)
    co = ChunkOpts(int(num_chunks), int(warmup), float(verify_tol))
    rep = ChunkReport()
    check(lib.moshii_sequence_solve(model.handle, prior.handle if prior is not None else None, C.byref(opts), n, descs,
                                    C.byref(co), BUFFERS_HOST | coop_group(coop), None, C.byref(rep)))
    del keep
    report = {k: getattr(rep, k) for k, _ in ChunkReport._fields_}
    return outs, report


def last_launch_info():
    name = C.create_string_buffer(128)
    lds = C.c_int32(0); thr = C.c_int32(0)
    load().moshii_last_launch_info(name, 128, C.byref(lds), C.byref(thr))
    return name.value.decode(), lds.value, thr.value


# ---- Stage-I (moshii_stagei_solve) -------------------------------------------------------------------------------
class StageIDesc(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('M', C.c_int32), ('n_faces', C.c_int32), ('nb', C.c_int32),
                ('faces', C.c_void_p), ('marker_vids', C.c_void_p), ('m2b', C.c_void_p), ('wt_init', C.c_void_p),
                ('n_obs', C.c_void_p), ('obs_ids', C.c_void_p), ('obs', C.c_void_p),
                ('exclude_vids', C.c_void_p), ('n_exclude', C.c_int32), ('betas_init', C.c_void_p),
                ('wt_data', C.c_double), ('wt_poseB', C.c_double), ('wt_poseH', C.c_double), ('wt_betas', C.c_double),
                ('wt_surf', C.c_double), ('annealing', C.c_void_p), ('n_anneal', C.c_int32),
                ('pose_ids', C.c_void_p), ('n_pose_ids', C.c_int32), ('body_ids', C.c_void_p), ('n_body', C.c_int32),
                ('finger_ids', C.c_void_p), ('n_finger', C.c_int32),
                ('n_expr', C.c_int32), ('expr_start', C.c_int32), ('face_ids', C.c_void_p), ('n_face', C.c_int32),
                ('wt_expr', C.c_double), ('wt_poseF', C.c_double),
                ('head_ids', C.c_void_p), ('head_corr', C.c_void_p), ('n_head', C.c_int32), ('n_head_rows', C.c_int32),
                ('wt_init_head', C.c_double), ('maxiter', C.c_int32), ('stagei_lr', C.c_double),
                ('sharded', C.c_int32), ('frame_lo', C.c_int32), ('frame_hi', C.c_int32), ('owns_shared_rows', C.c_int32),
                ('allreduce_sum', C.c_void_p), ('allreduce_user', C.c_void_p),
                ('betas', C.c_void_p), ('markers_latent', C.c_void_p), ('markers_latent_vids', C.c_void_p),
                ('pose', C.c_void_p), ('trans', C.c_void_p), ('markers_sim', C.c_void_p), ('expression', C.c_void_p),
                ('errs', C.c_void_p), ('iters', C.c_void_p), ('extra_initial_rigid_adjustment', C.c_int32),
                ('allreduce_on_device', C.c_int32), ('init_sq', C.c_void_p)]


ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_void_p)
STAGEI_ERR_NAMES = ('data', 'poseB', 'init', 'beta', 'surf', 'poseH', 'init_head_corr', 'poseF')   # 'beta' holds expr with n_expr > 0


def stagei_desc(NP, faces, marker_vids, m2b, wt_init, frames, nb, weights, pose_ids, body_ids, finger_ids=(), exclude_vids=None,
                betas_init=None, maxiter=100, stagei_lr=1e-3, head_corr=None, wt_init_head=None, frame_range=None,
                owns_shared_rows=True, allreduce=None, n_expr=0, expr_start=0, face_ids=(), extra_initial_rigid_adjustment=False,
                allreduce_on_device=False):
    """Fill a StageIDesc from NumPy data.  `frames`: list of (latent ids, obs[n,3]).  Returns (desc, outputs dict, keep-alive list)."""
    keep = []

    def ptr(a, dt):
        a = np.ascontiguousarray(a, dtype=dt); keep.append(a)
        return a.ctypes.data if a.size else None
    F, M = len(frames), len(marker_vids)
    d = StageIDesc()
    d.n_frames, d.M, d.n_faces, d.nb = F, M, len(faces), int(nb)
    d.faces = ptr(faces, np.int32); d.marker_vids = ptr(marker_vids, np.int32)
    d.m2b = ptr(m2b, np.float64); d.wt_init = ptr(wt_init, np.float64)
    d.n_obs = ptr([len(ids) for ids, _ in frames], np.int32)
    d.obs_ids = ptr(np.concatenate([np.asarray(ids) for ids, _ in frames]), np.int32)
    d.obs = ptr(np.vstack([np.asarray(o, dtype=np.float64).reshape(-1, 3) for _, o in frames]), np.float64)
    ex = np.zeros(0, np.int32) if exclude_vids is None else np.asarray(exclude_vids, np.int32)
    d.exclude_vids = ptr(ex, np.int32); d.n_exclude = len(ex)
    d.betas_init = ptr(np.asarray(betas_init, np.float64)[:nb], np.float64) if betas_init is not None else None
    d.wt_data, d.wt_poseB, d.wt_poseH = weights['stagei_wt_data'], weights['stagei_wt_poseB'], weights['stagei_wt_poseH']
    d.wt_betas, d.wt_surf = weights['stagei_wt_betas'], weights['stagei_wt_surf']
    ann = list(weights['stagei_wt_annealing'])
    d.annealing = ptr(ann, np.float64); d.n_anneal = len(ann)
    d.pose_ids = ptr(pose_ids, np.int32); d.n_pose_ids = len(pose_ids)
    d.body_ids = ptr(body_ids, np.int32); d.n_body = len(body_ids)
    d.finger_ids = ptr(list(finger_ids), np.int32); d.n_finger = len(finger_ids)
    d.maxiter, d.stagei_lr = int(maxiter), float(stagei_lr)
    d.extra_initial_rigid_adjustment = 1 if extra_initial_rigid_adjustment else 0
    d.n_expr, d.expr_start = int(n_expr), int(expr_start)
    d.face_ids = ptr(list(face_ids), np.int32); d.n_face = len(face_ids)
    d.wt_expr, d.wt_poseF = float(weights.get('stagei_wt_expr', 0.0)), float(weights.get('stagei_wt_poseF', 0.0))
    if head_corr is not None:
        hid, Cm = head_corr
        Cm = np.atleast_2d(np.asarray(Cm, np.float64))
        assert Cm.shape[1] == len(hid)
        d.head_ids = ptr(hid, np.int32); d.head_corr = ptr(Cm, np.float64); d.n_head, d.n_head_rows = Cm.shape[1], Cm.shape[0]
    d.wt_init_head = float(weights['stagei_wt_init'] if wt_init_head is None else wt_init_head)
    if allreduce is not None:
        # allreduce(array) sums a 1-D float64 NumPy array in place over the ranks (moshpp_amd.parallel.make_allreduce); with
        # allreduce_on_device it is allreduce(device_pointer, count) instead (parallel.make_allreduce_device: RCCL on the solver's
        # own buffers)
        def _cb(buf, count, _user):
            try:
                if allreduce_on_device:
                    allreduce(C.cast(buf, C.c_void_p).value, int(count))
                else:
                    allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:          # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = ALLREDUCE_CB(_cb)
        keep.append(cb)
        d.sharded = 1
        d.allreduce_on_device = 1 if allreduce_on_device else 0
        d.frame_lo, d.frame_hi = (0, F) if frame_range is None else (int(frame_range[0]), int(frame_range[1]))
        d.owns_shared_rows = 1 if owns_shared_rows else 0
        d.allreduce_sum = C.cast(cb, C.c_void_p)
    out = dict(betas=np.zeros(max(nb, 1)), markers_latent=np.zeros((M, 3)), markers_latent_vids=np.zeros(M, np.int32),
               pose=np.zeros((F, NP)), trans=np.zeros((F, 3)), markers_sim=np.zeros((F, M, 3)), expression=np.zeros((F, max(int(n_expr), 1))), errs=np.zeros(8),
               iters=np.zeros(1, np.int32), init_sq=np.zeros(M))
    for k, v in out.items():
        setattr(d, k, v.ctypes.data)
    out['betas'] = out['betas'][:nb]
    out['expression'] = out['expression'][:, :int(n_expr)]
    keep.append(out)
    return d, out, keep


EXPORTS['moshii_stagei_solve'] = (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(StageIDesc), C.c_void_p])


def stagei_solve_host(model: Model, prior, **kw):
    """moshii_stagei_solve on host buffers; kw as stagei_desc().  Returns dict(betas, markers_latent, markers_latent_vids, pose,
    trans, errs{term: SSE}, iters, init_sq[M]: every marker's share of errs['init'])."""
    require_device()
    desc, out, _keep = stagei_desc(NP=model.NP, **kw)
    check(load().moshii_stagei_solve(model.handle, prior.handle if prior is not None else None, C.byref(desc), None))
    out = dict(out)
    out['errs'] = dict(zip(STAGEI_ERR_NAMES, out['errs'].tolist()))
    out['iters'] = int(out['iters'][0])
    return out
