"""Measures the device's pow (through du_aug_gamma) and exp (through the blur weights of du_aug_blur) against fp64 on the GPU and
prints the two figures kept in tests/_augment_ref.py, E_POW_MEASURED and E_EXP_MEASURED (re-run after a ROCm update).
usage: python tools/measure_aug_intrinsics.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from dinounet_amd import _lib, ops

L = _lib.lib()
d = torch.device("cuda:0")
up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(d)
st = ops._st

# ---- pow
rs = np.random.RandomState(0)
n = 1 << 20
x = np.concatenate([rs.uniform(0, 1, n // 2), 10 ** rs.uniform(-6, 0, n // 2 - 2), [1.0, 0.5]]).astype(np.float32)
x = np.clip(x, 1e-6, 1.0).astype(np.float32)
gs = np.array([0.7, 0.85, 1.0, 1.2, 1.5], np.float32)
P = len(gs)
xs = np.tile(x, (P, 1))
stats = np.tile(np.array([0.5, 0.3, 0.0, 1.0], np.float32), (P, 1))
v, g_, i_, s_ = up(xs), up(gs), up(np.zeros(P)), up(stats)
_lib.check(L.du_aug_gamma(ops._p(v), ops._p(g_), ops._p(i_), ops._p(s_), P, n, st()), "gamma")
torch.cuda.synchronize()
out = v.cpu().numpy().astype(np.float64)
a32 = (x / (np.float32(1.0) + np.float32(1e-7))).astype(np.float32)
worst = 0.0
for p in range(P):
    ref = a32.astype(np.float64) ** np.float64(gs[p])
    e = np.abs(out[p] / ref - 1)
    print(f"pow g {gs[p]}: worst relative error {e.max():.4e} at a = {a32[e.argmax()]!r}")
    worst = max(worst, e.max())
print(f"E_POW_MEASURED {worst:.4e}  ({worst / 2 ** -24:.2f} U)")

# ---- exp through the blur weights
sig = np.concatenate([[0.374, 0.375, 0.625, 1.0], rs.uniform(0.5, 1.0, 64)]).astype(np.float32)
P, W, c = len(sig), 32, 16
x = np.zeros((P, 1, W), np.float32)
x[:, 0, c] = 1.0
xg, sg = up(x), up(sig)
y = torch.zeros_like(xg)
_lib.check(L.du_aug_blur(ops._p(xg), ops._p(y), ops._p(sg), P, 1, W, 1, st()), "blur")
torch.cuda.synchronize()
out = y.cpu().numpy().astype(np.float64)[:, 0]
worst = 0.0
for p in range(P):
    r = int(np.float32(4.0) * sig[p] + np.float32(0.5))
    for k in range(1, r + 1):
        a = -0.5 * k * k / np.float64(sig[p]) ** 2
        for side in (c + k, c - k):
            e = abs(out[p, side] / out[p, c] / np.exp(a) - 1) / (1 + abs(a))
            if e > worst:
                worst = e
                print(f"exp: sigma {sig[p]!r} k {k} a {a:.3f}: |w / exp(a) - 1| / (1 + |a|) = {e:.4e}")
print(f"E_EXP_MEASURED {worst:.4e}  ({worst / 2 ** -24:.2f} U)")
