"""An independent statement of how the f32 GEMM launchers choose: which kernel takes a descriptor, the split-K cut of inference and
of training, the column blocking nb and the K-tile depth of a single and of a grouped launch, when the GEMMs of a layer go out as
one launch, and how many slab groups the finish adds side by side.  Written from launch_gemm_mfma / launch_gemm_mfma_group as they
stood before the plan was factored out of them (csrc/kernels_fp32.hip at commit 11c5f16), in the order those functions tested
things; tests/test_gemm32_plan.py compares the library's plan (csrc/gemm32_plan.cpp, dumped by tools/pack_digest.cpp) against it.
A descriptor is a dict of the GemmDesc fields."""

ROUTES = ("none", "tiled_n1", "n1x4", "n1", "ci1", "mfma")   # the order of the library's enum
BM = 128


def ceil_div(a, b):
    return -(-a // b)


def route(d):
    if d["M"] == 0 or d["N"] == 0:
        return "none"
    if (d["N"] == 1 and d["nphx"] == 1 and d["TX"] == 3 and d["TY"] == 3 and d["CI"] == 8 and d["ax"] == 1 and d["bx"] == 1
            and d["ay"] == 1 and d["by"] == 1 and d["cx"] == -1 and d["cy"] == -1 and d["os"] == 1 and d["ox0"] == 0 and d["oy0"] == 0
            and d["OC"] == 1 and d["IH"] == d["OH"] and d["IW"] == d["OW"] and d["MH"] == d["OH"] and d["MW"] == d["OW"]
            and d["M"] > 0 and d["M"] % (d["MH"] * d["MW"]) == 0):
        return "tiled_n1"
    if (d["N"] == 1 and d["nphx"] == 1 and d["TX"] == 3 and d["TY"] == 3 and d["CI"] == 8 and d["ax"] == 1 and d["bx"] == 1
            and d["ay"] == 1 and d["os"] == 1 and d["ox0"] == 0 and d["OC"] == 1 and d["MW"] % 4 == 0 and d["OW"] % 4 == 0 and d["K"] <= 512):
        return "n1x4"
    if d["N"] == 1 and d["K"] <= 512 and d["nphx"] == 1:
        return "n1"
    if d["CI"] == 1 and d["N"] <= 8 and d["K"] <= 64 and d["nphx"] == 1 and d["CO"] == d["N"]:
        return "ci1"
    return "mfma"


def widest_nb(Npad):
    return 4 if Npad % 128 == 0 else (2 if Npad % 64 == 0 else 1)


def cut(d, batch_invariant):
    """(splits, kchunk) of the generic GEMM"""
    K, pix = d["K"], d["MH"] * d["MW"]
    if batch_invariant:
        if d["M"] == 0:
            return 1, K
        if pix == 1 and K >= 1024:
            return ceil_div(K, 256), 256
        if pix <= 64 and K >= 512:
            return ceil_div(K, 144), 144
        if pix <= 256 and K >= 512:
            return ceil_div(K, 256), 256
        return 1, K
    tiles = ceil_div(d["M"], BM) * (d["Npad"] // (32 * widest_nb(d["Npad"])))
    if tiles >= 128 or K < 256 or tiles == 0:
        return 1, K
    want = min(ceil_div(512, tiles), K // 64, 256)
    if want <= 1:
        return 1, K
    kchunk = ceil_div(ceil_div(K, want), 32) * 32
    return ceil_div(K, kchunk), kchunk


def tile(Npad, tiles):
    """(nb, BKT) of a launch with that many (row tile, K slab) pairs"""
    nb = widest_nb(Npad)
    while nb > 1 and tiles * (Npad // (32 * nb)) < 512:
        nb >>= 1
    return nb, (32 if tiles * (Npad // (32 * nb)) < 1024 else 16)


def single(d, batch_invariant):
    """One descriptor launched on its own: route, splits, kchunk, finish_groups, nb, bkt, vec, grid (x, y, z), finish grid x, slab floats"""
    r = route(d)
    o = dict(route=r, splits=1, kchunk=d["K"], finish_groups=1, nb=0, bkt=0, vec=0, grid=(0, 0, 0), fin=0, ws=0)
    M = d["M"]
    if r == "tiled_n1":
        o["grid"] = (ceil_div(d["OW"], 64), ceil_div(d["OH"], 16), M // (d["MH"] * d["MW"]))
    elif r == "n1x4":
        o["grid"] = (ceil_div(M // 4, 256), 1, 1)
    elif r in ("n1", "ci1"):
        o["grid"] = (ceil_div(M, 256), 1, 1)
    elif r == "mfma":
        splits, kchunk = cut(d, batch_invariant)
        rows = ceil_div(M, BM)
        nb, bkt = tile(d["Npad"], rows * splits)
        o.update(splits=splits, kchunk=kchunk, nb=nb, bkt=bkt, vec=int(d["K"] > 0 and d["CI"] % 4 == 0), grid=(rows, d["Npad"] // (32 * nb), splits))
        if splits > 1:
            total = M * d["N"]
            o["finish_groups"] = 8 if splits >= 32 and total < 65536 else 1
            o["fin"] = ceil_div(total, 256 // o["finish_groups"])
            o["ws"] = splits * M * d["Npad"]
    return o


def generic(d):
    """uses_generic_gemm: what a grouped launch asks of every member"""
    return d["M"] > 0 and d["N"] > 0 and d["K"] > 0 and route(d) == "mfma"


def group(ds, batch_invariant):
    """The GEMMs of one layer: (why they do not go out as one launch or None, the grouped launch or None, per-op dicts).  The
    reasons, in the order the launcher found them: count, member (a kernel other than the generic GEMM takes one), npad (mixed
    widths), ci4 (mixed gather forms), finish8 (one of them would be finished in 8 groups on its own)."""
    ops = [single(d, batch_invariant) for d in ds]
    why = None
    if not 2 <= len(ds) <= 4:
        why = "count"
    for d in ds:
        if why:
            break
        if not generic(d):
            why = "member"
        elif d["Npad"] != ds[0]["Npad"]:
            why = "npad"
        elif (d["CI"] % 4 == 0) != (ds[0]["CI"] % 4 == 0):
            why = "ci4"
    if not why and any(o["finish_groups"] == 8 for o in ops):
        why = "finish8"
    if why:
        for o in ops:
            o["slab_off"] = 0
        return why, None, ops
    tiles = sum(ceil_div(d["M"], BM) * o["splits"] for d, o in zip(ds, ops))
    Npad = ds[0]["Npad"]
    nb, bkt = tile(Npad, tiles)
    fins = [ceil_div(d["M"] * d["N"], 256) for d, o in zip(ds, ops) if o["splits"] > 1]
    launch = dict(nb=nb, bkt=bkt, vec=int(ds[0]["CI"] % 4 == 0), grid=(max(ceil_div(d["M"], BM) for d in ds), Npad // (32 * nb), sum(o["splits"] for o in ops)),
                  fin=(max(fins), len(ds)) if fins else (0, 0))
    off = 0
    for o in ops:
        o["slab_off"] = off
        off += o["ws"]
        o.update(nb=0, bkt=0, vec=0, grid=(0, 0, 0), fin=0)   # the members have no launch of their own
    return None, launch, ops
