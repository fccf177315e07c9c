"""TEST INFRASTRUCTURE: the MLP half of the simulated-DP buffer restated in numpy, one f32
rounding per operation (sgd_quantized_gradients.py:96-139, :381-404, :261-308 with
quantize_linear_grad / quantize_bias_grad :563-632, err_compensation=True, per channel):

  micro-step   v = g + e;  s == 0: s = max(max|v|, 1e-8) / qmax;  q = clamp(rint((1/s) * v + 0), -qmax-1, qmax)
               buf = buf + q;  e = v - q * s
  update       p = p + fl32(-lr) * (buf * (s / N))       (s / N a true division)
  zeroing      buf = 0, s = 0; e stays

plus the seeded gradients the fixture (tests/golden/make_golden_simdp_mlp.py) and the tests share,
and a kernels= implementation for dense.SimulatedDenseBuffers. Never used by the product."""
from __future__ import annotations

import numpy as np
import torch

f32 = np.float32

# (out, in): channel lengths 13, 5 | 64, 3 | 130, 4 | 1100, 2 | 5, 1 -- below a wave, exactly a
# wave, two waves and a tail, many iterations, a bias of one element
SHAPES = [(5, 13), (3, 64), (4, 130), (2, 1100), (1, 5)]
SEED = 2025
LR = 0.1
TIE_ROW = np.array([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, 3.0, -64.0, 100.5, -126.5, 7.25, -0.25, 31.0], f32)


def layer_params(shapes=SHAPES, seed=SEED):
    """[(W [out, in], b [out])], nn.Linear-like U(+-1/sqrt(in))."""
    rs = np.random.RandomState(seed)
    out = []
    for o, i in shapes:
        b = 1.0 / np.sqrt(i)
        out.append((rs.uniform(-b, b, (o, i)).astype(f32), rs.uniform(-b, b, o).astype(f32)))
    return out


def grads(window, k, shapes=SHAPES, seed=SEED):
    """[(gW, gb)] of micro-step k of a window. Per-row magnitudes spread over three decades.
    Micro-step 0: row 0 of layer 0 is TIE_ROW (max 127: s = 1 in the first window, rounding ties
    whose errors carry on) and row 1 of layer 1 is all zero (s = 1e-8/127, which must count as set).
    Micro-step 1 is 3.5 times micro-step 0 (values saturate at -128 / 127; the error keeps the
    rest). Later micro-steps are independent draws, the zero row included."""
    if k == 1:
        return [((f32(3.5) * gW).astype(f32), (f32(3.5) * gb).astype(f32)) for gW, gb in grads(window, 0, shapes, seed)]
    rs = np.random.RandomState(seed + 7919 * window + 104729 * k)
    out = []
    for j, (o, i) in enumerate(shapes):
        mag = (10.0 ** rs.uniform(-4, -1, (o, 1))).astype(f32)
        gW = (rs.standard_normal((o, i)) * mag).astype(f32)
        gb = (rs.standard_normal(o) * 10.0 ** rs.uniform(-3, -1)).astype(f32)
        if k == 0 and j == 0 and i == TIE_ROW.size:
            gW[0] = TIE_ROW
        if k == 0 and j == 1 and o > 1:
            gW[1] = 0.0
        out.append((gW, gb))
    return out


# ------------------------------------------------------------------ the arithmetic, one tensor
def ec_accumulate(g, e, buf, s, bits=8):
    """One micro-step of one tensor, in place on e, buf, s. Weight: g [out, in], s [out]; bias:
    g [out], s of one element (one channel)."""
    s1 = s.reshape(-1)
    g2, e2, b2 = (a.reshape(s1.size, -1) for a in (g, e, buf))
    n = f32(2 ** (bits - 1) - 1)
    v = (g2 + e2).astype(f32)
    unset = s1 == 0
    if unset.any():
        new = (np.maximum(np.abs(v).max(axis=1), f32(1e-8)) / n).astype(f32)
        s1[unset] = new[unset]
    r = (f32(1.0) / s1).astype(f32)[:, None]
    t = ((r * v).astype(f32) + f32(0.0)).astype(f32)
    q = np.clip(np.rint(t), -n - f32(1.0), n).astype(f32)
    b2[...] = (b2 + q).astype(f32)
    e2[...] = (v - (q * s1[:, None]).astype(f32)).astype(f32)


def sim_update(p, buf, s, num_gpus, lr):
    """The update of one tensor, in place on p."""
    s1 = s.reshape(-1)
    p2, b2 = p.reshape(s1.size, -1), buf.reshape(s1.size, -1)
    t = (s1 / f32(num_gpus)).astype(f32)[:, None]
    u = (f32(-lr) * (b2 * t).astype(f32)).astype(f32)
    p2[...] = (p2 + u).astype(f32)


class SimState:
    """scale / err / buf of a list of layers, per tensor: st[j] = dict(sw, sb, ew, eb, bw, bb)."""

    def __init__(self, shapes=SHAPES, bits=8):
        self.bits = bits
        self.st = [dict(sw=np.zeros(o, f32), sb=np.zeros(1, f32), ew=np.zeros((o, i), f32), eb=np.zeros(o, f32),
                        bw=np.zeros((o, i), f32), bb=np.zeros(o, f32)) for o, i in shapes]

    def micro_step(self, gs):
        for d, (gW, gb) in zip(self.st, gs):
            ec_accumulate(np.ascontiguousarray(gW, f32), d["ew"], d["bw"], d["sw"], self.bits)
            ec_accumulate(np.ascontiguousarray(gb, f32), d["eb"], d["bb"], d["sb"], self.bits)

    def update(self, params, num_gpus, lr):
        """params: [(W, b)] numpy arrays, updated in place."""
        for d, (W, b) in zip(self.st, params):
            sim_update(W, d["bw"], d["sw"], num_gpus, lr)
            sim_update(b, d["bb"], d["sb"], num_gpus, lr)

    def zero(self):
        for d in self.st:
            for k in ("sw", "sb", "bw", "bb"):
                d[k][...] = 0

    def flat(self, what):
        """scale [C] / err, buf [total] in dense.DenseChannels order (rows, then the bias, per layer)."""
        w, b = {"s": ("sw", "sb"), "e": ("ew", "eb"), "buf": ("bw", "bb")}[what]
        return np.concatenate([np.concatenate([d[w].reshape(-1), d[b].reshape(-1)]) for d in self.st])


# ------------------------------------------------------------------ kernels= for SimulatedDenseBuffers
class NumpySimKernels:
    """dense.SimulatedDenseKernels on the CPU over a DenseChannels table: the restatement above
    on the layers' own .grad / .data and the state tensors (CPU torch tensors share numpy's memory)."""

    def __init__(self, channels):
        self.ch = channels
        self.calls = []

    def prepare(self):
        self.calls.append("prepare")

    def _pieces(self):
        ch = self.ch
        for l, ws, bi in zip(ch.layers, ch.weight_slices, ch.bias_index):
            w0, b0 = int(ch.wire_off[ws.start]), int(ch.wire_off[bi])
            yield l.weight, slice(w0, w0 + l.weight.numel()), ws
            yield l.bias, slice(b0, b0 + l.bias.numel()), slice(bi, bi + 1)

    def ec_accumulate(self, bits, scale, err, buf):
        self.calls.append("ec_accumulate")
        s, e, b = scale.numpy(), err.numpy(), buf.numpy()
        for p, el, sl in self._pieces():
            ec_accumulate(p.grad.detach().numpy(), e[el].reshape(p.shape), b[el].reshape(p.shape), s[sl], bits)

    def sim_update(self, scale, buf, num_gpus, lr):
        self.calls.append("sim_update")
        s, b = scale.numpy(), buf.numpy()
        for p, el, sl in self._pieces():
            sim_update(p.data.numpy(), b[el].reshape(p.shape), s[sl], num_gpus, lr)


def torch_layers(shapes=SHAPES, seed=SEED, device="cpu"):
    """QuantLinear layers holding layer_params()."""
    from deep_quantized_recommendation_model_dqrm_amd import QuantLinear

    out = []
    for (o, i), (W, b) in zip(shapes, layer_params(shapes, seed)):
        lin = torch.nn.Linear(i, o)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(W))
            lin.bias.copy_(torch.from_numpy(b))
        q = QuantLinear(weight_bit=4, bias_bit=4, per_channel=True)
        q.set_param(lin)
        out.append(q.to(device))
    return out
