"""An independent statement of what a chunk of the 16-bit forward launches: the kernels in order, the ops each covers, the activation
buffers it reads and writes, M, gemm16's column blocking and split-K cut, every grid, mid16's workgroup shape and per-phase workgroup
counts, the tail's segmentation and workgroup count.  Written from run_encoder / run_gemm / fused_chunk / any16_chunk of
csrc/fused_bf16.hip and from the launchers of csrc/kernels_bf16.hip, kernels_mid16.hip, kernels_enc16.hip and kernels_any16.hip as
they stood before the plan was factored out of them (commit 56123b2), in the order those functions did things: `cur` is flipped by
hand, the integer codes 8 / 42 / 82 / 4 / 16 of mid16's shapes are formed and decoded again.  tests/test_lowp16_plan.py compares the
library's plan (csrc/lowp16_plan.cpp, dumped by tools/pack_digest.cpp --lowp16) against it.

One rule is stated differently from that code: run_gemm took a split only if its slabs fit the handle's slab buffer, which was sized
for the largest chunk the handle had seen (16 x chunk x 128 floats).  Here the buffer is the one a handle has whose largest call so
far is this chunk (`slab_elems`, default 16 c 128): the plan of a chunk must not depend on earlier calls.

An op is a dict(layer, Kpad, d) with d the GemmDesc fields; a switch set a dict of the Switches fields."""

KERNELS = ("enc_conv1_16", "enc16", "dense1_16", "gemm16", "gemm16n", "mid16", "tail16", "tail16s", "outconv16")   # the order of the library's enum
SHAPES = ("w4", "w8", "w16", "w4x2", "w8x2")                                                                       # the same of mid16's shapes
DEFAULT = dict(enc16=True, mid16=True, mid_shape=3, dense1_16=True, tail16s=False, mid_waves=0, tail_seg=0)
G_BP, G_BK = 128, 64          # kernels_bf16.hip
E_G = 5                       # kernels_enc16.hip: samples per workgroup of enc16
D1_NF = 144                   # kernels_enc16.hip: features per workgroup of dense1_16


def ceil_div(a, b):
    return -(-a // b)


def dense1_16_qualifies(d, Kpad):
    return d["MH"] == 1 and d["MW"] == 1 and d["K"] == 64 and Kpad == 64 and d["N"] == d["Npad"] and d["N"] % D1_NF == 0 and d["OC"] == d["N"] and d["CI"] == 64


def launch_gemm16(d, part, splits):
    wide = d["Npad"] % 128 == 0
    bn = 128 if wide else 64
    sk = splits > 1 and part
    kslice = d["K"]
    if sk:
        kslice = ceil_div(d["K"] // G_BK, splits) * G_BK
    nz = ceil_div(d["K"], kslice) if sk else 1
    out = dict(bn=bn, splits=splits if sk else 1, kslice=kslice, nz=nz, grid=(ceil_div(d["M"], G_BP), d["Npad"] // bn, nz), fin=0, slab=0)
    if sk:
        out["fin"] = ceil_div(d["M"] * (d["N"] // 4), 256)
        out["slab"] = nz * d["M"] * d["Npad"]          # the kernel writes slab z at part + z M Npad
    return out


def mid_template(sw):
    """(NW, PT) of the mid16 instantiation: fused_chunk's code, launch_mid16's decoding"""
    code = sw["mid_waves"] if sw["mid_waves"] else (8 if sw["mid_shape"] == 1 else 82 if sw["mid_shape"] == 2 else 42)
    if code == 4:
        return 4, 1
    if code == 16:
        return 16, 1
    if code == 42:
        return 4, 2
    if code == 82:
        return 8, 2
    return 8, 1


def tail_seg(sw, c, num_cus):
    seg = 1
    if sw["tail_seg"]:
        seg = sw["tail_seg"]
    else:
        best = ceil_div(c, num_cus) * 50 + 2
        for cand in (2, 5, 10, 25):
            cost = ceil_div(c * cand, num_cus) * (50 // cand + 1) + 2
            if cost * 115 < best * 100:
                best, seg = cost, cand
    return seg if seg in (1, 2, 5, 10, 25) else 1


def chunk(ops, fused, enc_ok, out_hw, sw, c, num_cus, slab_elems=None):
    """-> (steps, t1_buf, tail_seg); a step: dict(kernel, ops, src, dst) + what its launch takes.  src / dst: 0 / 1, 'x', 'y'."""
    part = 16 * c * 128 if slab_elems is None else slab_elems
    steps = []
    state = dict(cur=0, prev_layer=-1)

    def run_gemm(i, use_d1):
        o = ops[i]
        if o["layer"] != state["prev_layer"] and state["prev_layer"] >= 0:
            state["cur"] ^= 1
        state["prev_layer"] = o["layer"]
        d = dict(o["d"])
        d["M"] = c * d["MH"] * d["MW"]
        st = dict(ops=[i], src=state["cur"], dst=state["cur"] ^ 1, d=d)
        if use_d1 and o["layer"] == 4 and dense1_16_qualifies(d, o["Kpad"]):
            st.update(kernel="dense1_16", grid=(d["N"] // D1_NF,))
        elif d["CI"] % 64 != 0:
            st.update(kernel="gemm16n", grid=(ceil_div(d["M"], 128), d["Npad"] // 32))
        else:
            splits = 1
            if d["OH"] == 1 and d["OW"] == 1 and d["MH"] == 1 and d["MW"] == 1 and d["K"] >= 1024:
                splits = max(1, min(16, d["K"] // 256))
            if splits > 1 and splits * d["M"] * d["Npad"] > part:
                splits = 1
            st.update(kernel="gemm16", cut=launch_gemm16(d, part, splits))
        steps.append(st)

    use_enc = (enc_ok and sw["enc16"]) if fused else sw["enc16"]
    use_mid = fused and sw["mid16"]
    # run_encoder
    if not use_enc:
        steps.append(dict(kernel="enc_conv1_16", ops=[], src="x", dst=0, grid=(ceil_div(c * 25 * 16, 256),)))
    else:
        steps.append(dict(kernel="enc16", ops=[i for i, o in enumerate(ops) if o["layer"] < 4], src="x", dst=1, grid=(ceil_div(c, E_G),)))
        state["cur"] = 1
    for i, o in enumerate(ops):
        if use_enc and o["layer"] < 4:
            continue
        if use_mid and o["layer"] >= 5:
            break
        run_gemm(i, fused and sw["dense1_16"])
    if not fused:
        state["cur"] ^= 1
        steps.append(dict(kernel="outconv16", ops=[], src=state["cur"], dst="y", grid=(ceil_div(c * out_hw[0] * out_hw[1], 256),)))
        return steps, None, None
    if use_mid:
        state["cur"] ^= 1
        nw, pt = mid_template(sw)
        px = 32 * nw * pt                                  # MidCfg<NW, PT>::PX
        steps.append(dict(kernel="mid16", ops=[i for i, o in enumerate(ops) if o["layer"] >= 5], src=state["cur"], dst=state["cur"] ^ 1,
                          shape={(4, 1): "w4", (8, 1): "w8", (16, 1): "w16", (4, 2): "w4x2", (8, 2): "w8x2"}[(nw, pt)],
                          nblk=tuple(ceil_div(c * per, px) for per in (169, 156, 156, 144))))
    state["cur"] ^= 1
    seg = tail_seg(sw, c, num_cus)
    steps.append(dict(kernel="tail16s" if sw["tail16s"] else "tail16", ops=[], src=state["cur"], dst="y", seg=seg, blocks=min(c * seg, num_cus)))
    return steps, state["cur"], seg
