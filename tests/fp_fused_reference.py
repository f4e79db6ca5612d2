"""Plain numpy references for the four entry points of include/gaddpg.h section C.2 (gad_fp_rows, gad_fp_rows_grad,
gad_rows_act_out, gad_rows_act_bwd_stats), built from the references the operators they restate already have:
tests/fp_reference.py (three_interpolate and its gradient) and tests/layer_reference.py (the activation and the pooled-gradient
statistics).  tests/test_fp_fused_reference.py pins their composition to torch float64 autograd; tests/test_gpu_fp_fused.py holds
the kernels to them."""
import numpy as np

from tests import fp_reference as F
from tests import layer_reference as L

f32 = np.float32


def fp_rows(known_feats, idx, weight):
    """known_feats (B,C2,m), idx / weight (B,n,3) -> (B * n, C2) float32: gad_three_interpolate's output, transposed"""
    out = F.three_interpolate_ref(known_feats, idx, weight)                    # (B, C2, n)
    return np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(-1, out.shape[1])


def _channel_major(drows, B):
    drows = np.asarray(drows)
    return np.ascontiguousarray(drows.reshape(B, -1, drows.shape[1]).transpose(0, 2, 1))       # (B, C2, n)


def fp_rows_grad(drows, idx, weight, m, dtype=np.float64):
    """drows (B * n, C2) -> gknown_pm (B * m, C2): gad_three_interpolate_grad's sums, transposed (dtype float64: exact products)"""
    B = idx.shape[0]
    gp = F.three_interpolate_grad_ref(_channel_major(drows, B), idx, weight, m, dtype)          # (B, C2, m)
    return np.ascontiguousarray(gp.transpose(0, 2, 1)).reshape(B * m, -1)


def fp_rows_grad_bound(drows, idx, weight, m):
    """per destination element of gknown_pm: (cnt (B * m, 1) entries landing on the point, sum of |terms| (B * m, C2))"""
    B = idx.shape[0]
    cnt, mag = F.three_interpolate_grad_bound(_channel_major(drows, B), idx, weight, m)
    return cnt.reshape(B * m, 1), np.ascontiguousarray(mag.transpose(0, 2, 1)).reshape(B * m, -1)


def rows_act_out(z, scale, shift, B):
    """z (B * n, C) -> (B, C, n) float32 = relu(fmaf32(z, scale, shift)), transposed"""
    y = L.affine_act(z, scale, shift, 1)
    return np.ascontiguousarray(y.reshape(B, -1, y.shape[1]).transpose(0, 2, 1))


def rows_act_bwd_stats(dout, z, scale, shift, mean, istd, dtype):
    """dout (B,C,n), z (B * n, C): layer_reference.pool_bwd_stats with every row its own group -> its dict (masked = G (B * n, C))"""
    dout = np.asarray(dout, f32)
    rows = np.ascontiguousarray(dout.transpose(0, 2, 1)).reshape(-1, dout.shape[1])
    return L.pool_bwd_stats(rows, z, scale, shift, mean, istd, dtype)
