"""Generates tests/golden/ref_s2m.npz: the reference's own closed-form point-to-triangle distance and its gradients
(scan2mesh/mesh_distance/sample2meshdist.h:67-205, pointPlane / pointLine / pointPoint with Square), executed through
oracle/_ref/libs2m_ref.so (compiled in place by oracle/ref_build/Makefile) on the seeded points and mesh of
ref_inputs.surface_inputs(), each point against the triangle and nearest part the oracle finds for it.

Run in the build container only (needs the reference sources, or oracle/_ref/libs2m_ref.so already built); the npz is committed.
tests/test_ref_golden.py regenerates the inputs from the seeds and holds the oracle's distances and gradients to the recorded values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import stagei_oracle as s1  # noqa: E402
from tests.golden import ref_inputs  # noqa: E402

so_path = os.path.join(ROOT, 'oracle', '_ref', 'libs2m_ref.so')
if not os.path.exists(so_path):
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle', 'ref_build')])
lib = C.CDLL(so_path)
lib.s2m_ref_squared.restype = C.c_double
lib.s2m_ref_squared.argtypes = [C.c_int] + [C.POINTER(C.c_double)] * 8
P = C.POINTER(C.c_double)

si = ref_inputs.surface_inputs()
v, f, pts = si['v'], si['f'], si['pts']
_, tri, part, _, _, fv = s1.signed_surface_distance(pts, v, f, want_jac=True)
d2 = np.zeros(len(pts))
grad = np.zeros((len(pts), 4, 3))      # d(d^2) / d(point, a, b, c)
for i in range(len(pts)):
    x = np.ascontiguousarray(pts[i]); a, b, c = [np.ascontiguousarray(v[k]) for k in fv[i]]
    g = [np.zeros(3) for _ in range(4)]
    d2[i] = lib.s2m_ref_squared(int(part[i]), *[z.ctypes.data_as(P) for z in (x, a, b, c)], *[z.ctypes.data_as(P) for z in g])
    grad[i] = g
out = os.path.join(HERE, 'ref_s2m.npz')
np.savez(out, part=np.asarray(part, np.int32), tri_vertices=np.asarray(fv, np.int64), d2=d2, grad=grad)
print(f'wrote {out}: {len(pts)} points, nearest parts {sorted(set(int(p) for p in part))}')
