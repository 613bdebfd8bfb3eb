"""References for the model family (sr-for-cfd_amd/family.py) and for Conv2DTranspose(padding='same'), which oracle/ does not
restate.  Everything here is built from the oracle's own VALID pieces plus one crop:

    Keras / TF Conv2DTranspose(k, strides=s, padding='same'), k >= s, per axis:  out = in s,
    y = full[pb : pb + in s],  pb = (k - s) // 2,  full = the VALID result (no-flip scatter full[s i + a] += x[i] W[a]);
    bias and activation after the crop.

`convt_same_definition` is the definition the crop is checked against (tests/test_model_family.py): the gradient, with respect
to its input, of a SAME forward convolution (oracle.same_padding) whose input has in s rows, the kernel read as the forward
filter, by torch autograd in float64.
"""
import numpy as np

from oracle import sr_oracle as oracle


def convt_pb(k: int, s: int) -> int:
    return (k - s) // 2


def convt_same(x, w, b, stride=2, activation="linear"):
    """NHWC x, w (kh, kw, Cout, Cin): the crop rule on oracle.conv2d_transpose(valid)."""
    n, h, wd, _ = x.shape
    kh, kw, cout, _ = w.shape
    assert kh >= stride and kw >= stride
    full = oracle.conv2d_transpose(x, w, np.zeros(cout, x.dtype), stride, "valid", "linear")
    py, px = convt_pb(kh, stride), convt_pb(kw, stride)
    y = full[:, py:py + h * stride, px:px + wd * stride, :] + np.asarray(b).astype(x.dtype)
    return oracle._act(y, activation)


def convt_same_definition(x, w, stride):
    """float64: d/dX sum(conv2d_same(X, w) * x) for X of (in s) rows; no bias, no activation."""
    import torch
    import torch.nn.functional as F
    x = np.asarray(x, np.float64)
    n, h, wd, _ = x.shape
    kh, kw, cout, _ = w.shape
    X = torch.zeros((n, cout, h * stride, wd * stride), dtype=torch.float64, requires_grad=True)
    oh, pt, pb = oracle.same_padding(h * stride, kh, stride)
    ow, pl, pr = oracle.same_padding(wd * stride, kw, stride)
    assert (oh, ow) == (h, wd)
    wf = torch.tensor(np.asarray(w, np.float64)).permute(3, 2, 0, 1).contiguous()   # (kh,kw,Cin_fwd,Cout_fwd) -> (Cout_fwd,Cin_fwd,kh,kw)
    Y = F.conv2d(F.pad(X, (pl, pr, pt, pb)), wf, None, stride=stride)
    (Y * torch.tensor(x).permute(0, 3, 1, 2)).sum().backward()
    return X.grad.permute(0, 2, 3, 1).numpy()


def forward_specs64(specs, x, dtype=np.float64):
    """float64 forward of a spec graph (`SRModel.from_layers` dicts), NHWC."""
    h = np.asarray(x, dtype)
    for s in specs:
        kind = s["kind"]
        if kind == "flatten":
            h = h.reshape(h.shape[0], 1, 1, -1)
        elif kind == "reshape":
            h = h.reshape((h.shape[0],) + tuple(s["shape"]))
        elif kind == "dense":
            h = oracle.dense(h.reshape(h.shape[0], -1), np.asarray(s["w"]), np.asarray(s["b"]), s.get("act", "linear"))
            h = h.reshape(h.shape[0], 1, 1, -1)
        elif kind == "conv2d":
            h = oracle.conv2d(h, np.asarray(s["w"]), np.asarray(s["b"]), int(s.get("stride", 1)), "same" if s.get("same") else "valid", s.get("act", "linear"))
        elif kind == "conv2d_transpose":
            st = int(s.get("stride", 1))
            if s.get("same"):
                h = convt_same(h, np.asarray(s["w"]), np.asarray(s["b"]), st, s.get("act", "linear"))
            else:
                h = oracle.conv2d_transpose(h, np.asarray(s["w"]), np.asarray(s["b"]), st, "valid", s.get("act", "linear"))
        else:
            raise ValueError(kind)
    return h


def macs(specs, in_shape) -> int:
    """Multiply-accumulates per sample: for a transposed convolution the (input pixel, tap) pairs that land inside the output."""
    h, w, c = in_shape
    total = 0
    for s in specs:
        kind = s["kind"]
        if kind == "flatten":
            h, w, c = 1, 1, h * w * c
        elif kind == "reshape":
            h, w, c = s["shape"]
        elif kind == "dense":
            cin, cout = np.asarray(s["w"]).shape
            total += cin * cout
            h, w, c = 1, 1, cout
        elif kind == "conv2d":
            kh, kw, cin, cout = np.asarray(s["w"]).shape
            st = int(s.get("stride", 1))
            oh, ow = (-(-h // st), -(-w // st)) if s.get("same") else ((h - kh) // st + 1, (w - kw) // st + 1)
            total += oh * ow * kh * kw * cin * cout
            h, w, c = oh, ow, cout
        else:
            kh, kw, cout, cin = np.asarray(s["w"]).shape
            st = int(s.get("stride", 1))

            def axis(n, k):
                if not s.get("same"):
                    return n * k, (n - 1) * st + k
                pb = convt_pb(k, st)
                return sum(1 for i in range(n) for a in range(k) if pb <= st * i + a < pb + n * st), n * st
            (py, oh), (px, ow) = axis(h, kh), axis(w, kw)
            total += py * px * cin * cout
            h, w, c = oh, ow, cout
    return total


# ---------------------------------------------------------------------------
# gradients: torch autograd of F.conv_transpose2d + the crop
# ---------------------------------------------------------------------------
def _forward_torch(specs, params, x, dtype, pre=None):
    import torch
    import torch.nn.functional as F
    from oracle.sr_oracle_autograd import _act_t

    def act(z, s):
        if pre is not None:
            z.retain_grad()
            pre.append(z)
        return _act_t(z, s.get("act", "linear"))

    h = torch.as_tensor(np.asarray(x), dtype=dtype).permute(0, 3, 1, 2)
    for i, s in enumerate(specs):
        kind = s["kind"]
        if kind == "flatten":
            h = h.permute(0, 2, 3, 1).reshape(h.shape[0], -1)
        elif kind == "reshape":
            oh, ow, oc = s["shape"]
            h = h.reshape(h.shape[0], oh, ow, oc).permute(0, 3, 1, 2)
        elif kind == "dense":
            w, b = params[i]
            h = act(h @ w + b, s)
        elif kind == "conv2d":
            w, b = params[i]
            st = int(s.get("stride", 1))
            if s.get("same", False):
                _, pt, pb = oracle.same_padding(h.shape[2], w.shape[0], st)
                _, pl, pr = oracle.same_padding(h.shape[3], w.shape[1], st)
                h = F.pad(h, (pl, pr, pt, pb))
            h = act(F.conv2d(h, w.permute(3, 2, 0, 1).contiguous(), b, stride=st), s)
        elif kind == "conv2d_transpose":
            w, b = params[i]
            st = int(s.get("stride", 1))
            ih, iw = h.shape[2], h.shape[3]
            full = F.conv_transpose2d(h, w.permute(3, 2, 0, 1).contiguous(), None, stride=st)
            if s.get("same", False):
                py, px = convt_pb(w.shape[0], st), convt_pb(w.shape[1], st)
                full = full[:, :, py:py + ih * st, px:px + iw * st]
            h = act(full + b.reshape(1, -1, 1, 1), s)
        else:
            raise ValueError(kind)
    return h.permute(0, 2, 3, 1) if h.dim() == 4 else h


def _loss_and_grads(specs, x, y, dtype, bias_cond=False):
    import torch
    params = {i: (torch.tensor(np.asarray(s["w"]), dtype=dtype, requires_grad=True), torch.tensor(np.asarray(s["b"]), dtype=dtype, requires_grad=True))
              for i, s in enumerate(specs) if "w" in s}
    pre = [] if bias_cond else None
    pred = _forward_torch(specs, params, x, dtype, pre)
    yt = torch.as_tensor(np.asarray(y), dtype=dtype).reshape(pred.shape)
    loss = torch.mean((yt - pred) ** 2)
    loss.backward()
    flat = np.concatenate([t.grad.numpy().astype(np.float64).reshape(-1) for i in sorted(params) for t in params[i]])
    if not bias_cond:
        return float(loss.item()), flat
    conds = []
    for z in pre:
        g = z.grad.double().transpose(0, 1).reshape(z.shape[1], -1)
        conds.append(float(torch.linalg.norm(g.abs().sum(1)) / max(float(torch.linalg.norm(g.sum(1))), 1e-300)))
    return float(loss.item()), flat, conds


class GradRef:
    """What tests/test_gpu_training_oracle.py's `Ref` holds (l64, g64, cond, l32, g32, sizes), for graphs with padding='same'
    transposed convolutions: that module's `check` applies unchanged."""

    def __init__(self, specs, in_shape, x, y):
        import torch
        from oracle import sr_oracle_autograd as ag
        assert tuple(np.asarray(x).shape[1:]) == tuple(in_shape)
        self.l64, self.g64, self.cond = _loss_and_grads(specs, x, y, torch.float64, bias_cond=True)
        self.l32, self.g32 = _loss_and_grads(specs, x, y, torch.float32)
        self.sizes = ag.param_sizes_specs(specs)


# ---------------------------------------------------------------------------
# 16-bit emulation: the rounding rules of oracle/sr_oracle_lowp.py (rs, r, q, q_div, q_mul) on any spec graph
# ---------------------------------------------------------------------------
def forward_specs_lowp(specs, x, kind="bf16"):
    """What the 16-bit path computes up to accumulation order and the hardware exp / rcp: weights and the activations handed from
    one layer to the next rounded to `kind`, sums in float64.  The first layer runs on unrounded weights (a vector kernel in
    f32), the last layer's output is not rounded.  Swish outputs are stored as round(log2e a); a linear layer that consumes them
    uses round(W / log2e) (q_div), a swish layer behind a linear one round(W log2e) (q_mul), otherwise round(W) (q)."""
    from oracle import sr_oracle_lowp as lp
    LOG2E = lp.LOG2E
    rnd = lp.round_bf16 if kind == "bf16" else lp.round_f16
    q = lambda w: rnd(w).astype(np.float64)
    q_div = lambda w: LOG2E * rnd(np.asarray(w, np.float64) / LOG2E).astype(np.float64)
    q_mul = lambda w: rnd(np.asarray(w, np.float64) * LOG2E).astype(np.float64) / LOG2E
    r = lambda a: rnd(a.astype(np.float32)).astype(np.float64)
    rs = lambda a: rnd((a * LOG2E).astype(np.float32)).astype(np.float64) / LOG2E
    weighted = [i for i, s in enumerate(specs) if "w" in s]
    h = np.asarray(x, np.float64)
    prev_swish = False
    for i, s in enumerate(specs):
        kind_, act = s["kind"], s.get("act", "linear")
        if kind_ == "flatten":
            h = h.reshape(h.shape[0], 1, 1, -1)
            continue
        if kind_ == "reshape":
            h = h.reshape((h.shape[0],) + tuple(s["shape"]))
            continue
        swish = act in ("swish", "silu")
        w = np.asarray(s["w"])
        if i == weighted[0]:
            wq = w.astype(np.float64)
        elif prev_swish and not swish:
            wq = q_div(w)
        elif swish and not prev_swish:
            wq = q_mul(w)
        else:
            wq = q(w)
        one = [dict(s, w=wq, b=np.asarray(s["b"], np.float64))]
        h = forward_specs64(one, h)
        if i != weighted[-1]:
            h = rs(h) if swish else r(h)
        prev_swish = swish
    return h


def forward_specs_lowp2(specs, x, kind="bf16"):
    """The second emulation of a spec graph (error_maps.second_emulation, which is written for encoder_10 + decoder_400, on any
    graph `forward_specs_lowp` takes): the same roundings of weights and of the activations handed from layer to layer, and only
    what the device is allowed to differ in differs -- float32 accumulation one product at a time in a permuted channel order
    (error_maps._mm_seq), taps in reverse order, bias first, exp2 / reciprocal a few ulp off (error_maps._swish).  As on the
    device, a swish layer's sum arrives scaled by log2(e) (its weights and bias carry the factor) and its stored output keeps it."""
    import error_maps as em
    from oracle import sr_oracle_lowp as lp
    f32 = np.float32
    LOG2E = lp.LOG2E
    rnd = lp.round_bf16 if kind == "bf16" else lp.round_f16
    rng = np.random.default_rng(77)
    q = lambda w: rnd(np.asarray(w, f32))
    q_div = lambda w: rnd((np.asarray(w, np.float64) / LOG2E).astype(f32))
    q_mul = lambda w: rnd((np.asarray(w, np.float64) * LOG2E).astype(f32))

    def conv_same(a, w, b, stride, same):
        n, h, wd, _ = a.shape
        kh, kw, _, cout = w.shape
        if same:
            oh, pt, pb = oracle.same_padding(h, kh, stride)
            ow, pl, pr = oracle.same_padding(wd, kw, stride)
            a = np.pad(np.asarray(a, f32), ((0, 0), (pt, pb), (pl, pr), (0, 0)))
        else:
            oh, ow = (h - kh) // stride + 1, (wd - kw) // stride + 1
        out = np.zeros((n, oh, ow, cout), f32) + b
        for ky in reversed(range(kh)):
            for kx in reversed(range(kw)):
                out += em._mm_seq(a[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride], w[ky, kx])
        return out

    def conv_t(a, w, b, stride, same):
        n, h, wd, _ = a.shape
        kh, kw, cout, _ = w.shape
        out = np.zeros((n, (h - 1) * stride + kh, (wd - 1) * stride + kw, cout), f32) + b
        for ky in reversed(range(kh)):
            for kx in reversed(range(kw)):
                out[:, ky:ky + (h - 1) * stride + 1:stride, kx:kx + (wd - 1) * stride + 1:stride] += em._mm_seq(a, w[ky, kx].T)
        if same:
            py, px = convt_pb(kh, stride), convt_pb(kw, stride)
            out = out[:, py:py + h * stride, px:px + wd * stride]
        return out

    weighted = [i for i, s in enumerate(specs) if "w" in s]
    h = np.asarray(x, f32)
    prev_swish = False
    for i, s in enumerate(specs):
        kind_ = s["kind"]
        if kind_ == "flatten":
            h = h.reshape(h.shape[0], 1, 1, -1)
            continue
        if kind_ == "reshape":
            h = h.reshape((h.shape[0],) + tuple(s["shape"]))
            continue
        swish = s.get("act", "linear") in ("swish", "silu")
        first = i == weighted[0]
        if first:
            w = np.asarray(s["w"], f32)          # a vector kernel in f32 on unrounded weights; the factor goes onto the sum
        elif prev_swish and not swish:
            w = q_div(s["w"])
        elif swish and not prev_swish:
            w = q_mul(s["w"])
        else:
            w = q(s["w"])
        b = np.asarray(s["b"], f32) * (f32(LOG2E) if swish and not first else f32(1))
        st = int(s.get("stride", 1))
        if kind_ == "dense":
            pre = (em._mm_seq(h.reshape(h.shape[0], -1), w) + b).reshape(h.shape[0], 1, 1, -1)
        elif kind_ == "conv2d":
            pre = conv_same(h, w, b, st, bool(s.get("same")))
        elif kind_ == "conv2d_transpose":
            pre = conv_t(h, w, b, st, bool(s.get("same")))
        else:
            raise ValueError(kind_)
        if swish:
            h = rnd(em._swish(pre * f32(LOG2E) if first else pre, rng, True))
        else:
            h = pre if i == weighted[-1] else rnd(pre)
        prev_swish = swish
    return h.astype(np.float64) / (LOG2E if prev_swish else 1.0)
