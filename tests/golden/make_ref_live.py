"""Writes tests/golden/ref_kernels_live.npz: what the reference's own kernels (oracle/_ref, built by ``make -C oracle ref``
from a reference checkout) produce on the inputs of the GPU tests that compare the HIP kernels with them at full size
(tests/test_gpu_parity.py::test_pairwise_op_vs_reference_kernels_live_full_size, tests/test_gpu_tree_filter.py::
test_refine_vs_reference_kernels_live_96x96 and ::test_large_refine_vs_reference_kernels_live_200x304), so that those tests
run where oracle/_ref is not built.

  * pairwise_nlog at 32 x 200 x 256 (size 3, dilation 2): the sha256 of the forward and backward outputs (52 MB; the tests
    recompute them with the C oracle, which must reproduce them bit for bit);
  * tree-filter refine at 96 x 96 and 200 x 304: forward output, feature gradient and per-vertex edge-weight gradient on the
    reference Boruvka tree of the seeded feature map, plus the sha256 of that tree's sorted edge list.

    python tests/golden/make_ref_live.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import pairwise_ref as pr  # noqa: E402
from oracle import tree_filter_oracle as tfo  # noqa: E402


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tree_digest(tree) -> str:
    e = np.sort(np.asarray(tree, np.int64).reshape(-1, 2), axis=1)
    return digest(e[np.lexsort((e[:, 1], e[:, 0]))])


def pairwise_inputs():
    rng = np.random.default_rng(5)
    x = (2.5 * rng.standard_normal((32, 1, 200, 256))).astype(np.float32)
    gp = rng.random((32, 8, 200, 256)).astype(np.float32)
    return x, gp


def refine_inputs(seed, H, W, C):
    """the tests' draw order: feature map, then (the tree in between) x, g, per-vertex edge weights"""
    rng = np.random.default_rng(seed)
    fm = rng.standard_normal((3, H, W)).astype(np.float32)
    V = H * W
    x = rng.standard_normal((C, V)).astype(np.float32)
    g = rng.standard_normal((C, V)).astype(np.float32)
    w_vertex = np.exp(-rng.random(V) * 0.8).astype(np.float32)
    return fm, x, g, w_vertex


def ref_refine(tree, x, g, w_vertex, V):
    r_si, r_sp, r_sc = tfo.ref_bfs(tree, V)
    fwd = tfo.ref_refine_forward(x, w_vertex[r_si], r_si, r_sp, r_sc)
    r_gf, r_gw = tfo.ref_refine_backward(g, w_vertex[r_si], r_si, r_sp, r_sc, fwd)
    want_gw = np.zeros(V, np.float32)
    want_gw[r_si] = r_gw
    return fwd['out'], r_gf, want_gw


if __name__ == '__main__':
    assert pr.available() and tfo.ref_available() and tfo.ref_kernels_available(), 'make -C oracle ref first'
    out = {}
    x, gp = pairwise_inputs()
    want = pr.forward(x, 3, 2)
    out['pw_full_fwd_sha256'] = np.array(digest(want))
    out['pw_full_bwd_sha256'] = np.array(digest(pr.backward(x, want, gp, 3, 2)))
    for name, seed, H, W, C in (('tf96', 77, 96, 96, 2), ('tf200x304', 78, 200, 304, 1)):
        fm, x, g, w_vertex = refine_inputs(seed, H, W, C)
        idx = tfo.grid_edges(H, W)
        tree = tfo.ref_boruvka_mst(idx, tfo.grid_weights(fm), H * W)
        o, gf, gw = ref_refine(tree, x, g, w_vertex, H * W)
        out.update({f'{name}_tree_sha256': np.array(tree_digest(tree)), f'{name}_out': o, f'{name}_gf': gf, f'{name}_gw': gw})
    np.savez_compressed(os.path.join(HERE, 'ref_kernels_live.npz'), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()})
