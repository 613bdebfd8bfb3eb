"""An independent statement of how the split-bf16 GEMM launchers choose (SRCFD_PREC_FP32X3): which descriptors the kernels take, which
ops the weights-resident kernel takes, when the GEMMs of a layer go out as one launch, every grid, the group's table of first
workgroups and the resident kernel's tile count.  Written from launch_gemm_x3 / launch_gemm_x3_group as they stood before the plan
was factored out of them (csrc/kernels_x3.hip at commit 3bd6482), in the order those functions tested things;
tests/test_x3_forms.py compares the library's plan (csrc/x3_plan.cpp, dumped by tools/pack_digest.cpp --forms) against it, and
tests/test_gpu_x3_forms.py asks it what the table's cases reach on the device's own CU count.  A descriptor is a dict of the
GemmDesc fields; `descriptors` restates how the engine derives them from a layer (build_plan, csrc/operand_pack.cpp), so that the
device test needs no dump, and the CPU test holds it to the dumped ones."""

KERNELS = ("tile", "res")   # the order of the library's enum
BP, BN, BK = 128, 128, 32
RES_K = 128
SWISH, LINEAR = 1, 0        # include/srcfd.h


def ceil_div(a, b):
    return -(-a // b)


def qualifies(d):
    if not (d["K"] >= 128 and d["CI"] % BK == 0 and d["N"] % BN == 0 and d["CO"] % 32 == 0 and d["OC"] % 4 == 0 and d["act"] in (SWISH, LINEAR)):
        return False
    if d["M"] <= 0:
        return True
    images = d["M"] // (d["MH"] * d["MW"]) + 1
    return images * d["IH"] * d["IW"] * d["CI"] < 2 ** 31 and images * d["OH"] * d["OW"] * d["OC"] < 2 ** 31


def res_qualifies(d):
    return d["K"] <= RES_K and d["K"] % BK == 0 and d["TY"] * d["TX"] == 1 and d["cy"] == 0 and d["cx"] == 0


def kpad(d):
    return ceil_div(d["K"], BK) * BK


def single(d, num_cus):
    """one descriptor launched on its own: kernel, kpad, grid (x, y), ntiles"""
    o = dict(kernel="res" if res_qualifies(d) else "tile", kpad=kpad(d), grid=(0, 0), ntiles=0)
    if d["M"] <= 0:
        return o
    if o["kernel"] == "res":
        ntiles, nblk = ceil_div(d["M"], 32), d["N"] // BN
        o.update(ntiles=ntiles, grid=(max(1, min(ceil_div(ntiles, 8), max(1, num_cus // nblk))), nblk))
    else:
        o["grid"] = (ceil_div(d["M"], BP), d["N"] // BN)
    return o


def group(ds, num_cus):
    """The GEMMs of one layer: (why they do not go out as one launch or None, (group grid, first[5]) or None, per-op dicts).  The
    reasons, in the order the launcher found them: count, then member (an op is empty or the resident kernel takes it)."""
    ops = [single(d, num_cus) for d in ds]
    why = None if 2 <= len(ds) <= 4 else "count"
    for d in ds:
        if why:
            break
        if d["M"] <= 0 or res_qualifies(d):
            why = "member"
    if why:
        return why, None, ops
    first, total = [], 0
    for d in ds:
        first.append(total)
        total += ceil_div(d["M"], BP) * (d["N"] // BN)
    return None, (total, tuple(first + [total] * (5 - len(ds)))), ops


FIELDS = "M N K Npad MH MW TY TX CI IH IW ay by cy ax bx cx CO nphx OH OW OC os oy0 ox0 act".split()
ACT = {"linear": 0, "swish": 1, "relu": 2, "sigmoid": 3, "tanh": 4}   # include/srcfd.h


def descriptors(L, ih, iw, n):
    """The GEMMs of one layer of tests/gemm32_forms.py's layer dicts on an (ih, iw, cin) input at batch n: one, or one per output
    phase of a transposed convolution whose kernel is not its stride."""
    kh, kw, s, cin, cout = L["kh"], L["kw"], L["stride"], L["cin"], L["cout"]
    d = dict.fromkeys(FIELDS, 0)
    d.update(act=ACT[L["act"]], OC=cout, CO=cout, nphx=1, os=1, IH=ih, IW=iw, CI=cin, N=cout)
    if L["kind"] == "dense":
        d.update(IH=1, IW=1, OH=1, OW=1, MH=1, MW=1, TY=1, TX=1, K=cin)
        out = [d]
    elif L["kind"] == "conv2d":
        oh, ow = (ceil_div(ih, s), ceil_div(iw, s)) if L["same"] else ((ih - kh) // s + 1, (iw - kw) // s + 1)
        pt = max((oh - 1) * s + kh - ih, 0) // 2 if L["same"] else 0   # TF SAME: the extra pixel goes after
        pl = max((ow - 1) * s + kw - iw, 0) // 2 if L["same"] else 0
        d.update(OH=oh, OW=ow, MH=oh, MW=ow, TY=kh, TX=kw, ay=s, ax=s, by=1, bx=1, cy=-pt, cx=-pl, K=kh * kw * cin)
        out = [d]
    else:
        assert L["kind"] == "conv2d_transpose"
        oh, ow = (ih * s, iw * s) if L["same"] else ((ih - 1) * s + kh, (iw - 1) * s + kw)
        d.update(OH=oh, OW=ow)
        if (kh, kw) == (s, s):   # kernel == stride: the phases are column groups of one GEMM
            d.update(MH=ih, MW=iw, TY=1, TX=1, ay=1, ax=1, K=cin, N=s * s * cout, nphx=s, os=s)
            out = [d]
        else:
            pby, pbx = ((kh - s) // 2, (kw - s) // 2) if L["same"] else (0, 0)
            out = []
            for py in range(s):
                for px in range(s):
                    ry, rx = (py - pby) % s, (px - pbx) % s
                    p = dict(d, TY=ceil_div(kh - py, s) if py < kh else 0, TX=ceil_div(kw - px, s) if px < kw else 0,
                             MH=ceil_div(oh - ry, s) if ry < oh else 0, MW=ceil_div(ow - rx, s) if rx < ow else 0)
                    if p["MH"] == 0 or p["MW"] == 0:
                        continue
                    p.update(ay=1, ax=1, by=-1, bx=-1, cy=(ry + pby - py) // s, cx=(rx + pbx - px) // s, os=s, oy0=ry, ox0=rx)
                    p["K"] = p["TY"] * p["TX"] * cin
                    out.append(p)
    for p in out:
        p.update(Npad=ceil_div(p["N"], 32) * 32, M=n * p["MH"] * p["MW"])
    return out
