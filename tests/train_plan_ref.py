"""An independent statement of the training step's weight-gradient plan: the forward GEMM descriptors of a layer graph
(csrc/operand_pack.cpp build_plan), the slab count of each weight-gradient launch (wgrad_plan) and the tier of slab groups the one
slab-sum launch uses for it (finish_groups).  Written for tests/test_gpu_training_oracle.py, which uses it to PROVE which tier a
case reaches; tests/test_train_plan.py compares the library's plan (plan_step, dumped by tools/pack_digest.cpp) against it."""


def gemm_ops(specs, in_shape):
    h, w, c = in_shape
    ops = []
    for s in specs:
        kind, name = s["kind"], s.get("name")
        if kind == "flatten":
            h, w, c = 1, 1, h * w * c
            continue
        if kind == "reshape":
            h, w, c = s["shape"]
            continue
        if kind == "dense":
            cin, cout = s["w"].shape
            ops.append(dict(layer=name, K=cin, N=cout, MH=1, MW=1, TY=1, TX=1, CI=cin, nphx=1))
            h, w, c = 1, 1, cout
        elif kind == "conv2d":
            k, st, cin, cout = s["w"].shape[0], s.get("stride", 1), s["w"].shape[2], s["w"].shape[3]
            oh, ow = (-(-h // st), -(-w // st)) if s.get("same") else ((h - k) // st + 1, (w - k) // st + 1)
            ops.append(dict(layer=name, K=k * k * cin, N=cout, MH=oh, MW=ow, TY=k, TX=k, CI=cin, nphx=1))
            h, w, c = oh, ow, cout
        else:
            k, st, cout, cin = s["w"].shape[0], s["stride"], s["w"].shape[2], s["w"].shape[3]
            oh, ow = (h - 1) * st + k, (w - 1) * st + k
            if k == st:
                ops.append(dict(layer=name, K=cin, N=st * st * cout, MH=h, MW=w, TY=1, TX=1, CI=cin, nphx=st))
            else:
                for py in range(st):
                    for px in range(st):
                        ty = -(-(k - py) // st) if py < k else 0
                        tx = -(-(k - px) // st) if px < k else 0
                        mh = -(-(oh - py) // st) if py < oh else 0
                        mw = -(-(ow - px) // st) if px < ow else 0
                        if mh and mw:
                            ops.append(dict(layer=name, K=ty * tx * cin, N=cout, MH=mh, MW=mw, TY=ty, TX=tx, CI=cin, nphx=1))
            h, w, c = oh, ow, cout
    return ops


def wgrad_slices(d, n):
    """(slices, rows per slice, M) of wgrad_plan for op d at batch n."""
    M = n * d["MH"] * d["MW"]
    if d["N"] == 1 and d["TY"] == 3 and d["TX"] == 3 and d["CI"] == 8 and d["nphx"] == 1:   # wgrad_is_n1_k72
        ns = max(1, min(256, (M + 1023) // 1024))
        rps = -(-M // ns)
        return max(1, -(-M // rps)), rps, M
    ktiles = (d["K"] + 1 + 31) // 32
    ntiles = -(-d["N"] // 32)
    KG = 2 if ktiles >= 2 else 1
    NG = 4 if ntiles >= 3 else (2 if ntiles == 2 else 1)
    blocks = -(-ktiles // KG) * -(-ntiles // NG)
    chunks = max(1, -(-M // 64))
    want = max(1, min(chunks, 512 // blocks))
    rps = -(-chunks // want) * 64
    return max(1, -(-M // rps)), rps, M


def short_last_slice(d, n):
    """whether op d's last weight-gradient slice at batch n has fewer rows than the others"""
    ns, rps, M = wgrad_slices(d, n)
    return ns > 1 and M % rps != 0


# ---------------------------------------------------------------------------
# The three rules of the SR network's step that move with the batch n beside the slices above (tests/train_batches.py,
# tests/test_gpu_train_batches.py: what Trainer.last_step() must report, and which batches reach which form)
# ---------------------------------------------------------------------------
def tail32_segments(n, H, cus):
    """Segments per sample of the fused tail's forward launch (kernels_tail32.hip): a sample is 2H strips; the busiest workgroup
    walks ceil(n S / cus) virtual samples of ceil(2H / S) + 1 strips, + 2 rounds of pipeline depth; a larger S is taken only
    where it is more than 10 % cheaper than the best so far."""
    strips = 2 * H
    best, seg = -(-n // cus) * strips + 2, 1
    for cand in range(2, strips + 1):
        cost = -(-n * cand // cus) * (-(-strips // cand) + 1) + 2
        if cost * 110 < best * 100:
            best, seg = cost, cand
    return seg


def tail32_ragged(n, H, cus):
    """the segment count does not divide the strip count: segments of two different lengths"""
    return (2 * H) % tail32_segments(n, H, cus) != 0


def tail32_blocks(n, seg, cus):
    """workgroups of that launch: one per virtual sample, at most one per CU"""
    return min(n * max(seg, 1), cus)


def tail_bwd32_tiles(n, H, W):
    """(16-pixel tiles of the fused tail's backward launch over the n H W pixels of its input level, pixels of the last tile,
    pairs of tiles: a workgroup takes two tiles at a time)"""
    px = n * H * W
    tiles = -(-px // 16)
    return tiles, px - 16 * (tiles - 1), (tiles + 1) // 2


def tail_bwd32_blocks(n, H, W, cus):
    """workgroups (= weight-gradient slabs) of that launch"""
    return max(1, min(tail_bwd32_tiles(n, H, W)[2], cus))


def train_enc_groups(n):
    """(full groups of 16 samples, samples of the partial last group) of the fused encoder's first launch"""
    return n // 16, n % 16


def tier(slices):
    """finishing groups wgrad_finish_all_f32 uses for that many slabs"""
    return 32 if slices >= 256 else (8 if slices >= 64 else (4 if slices >= 8 else 1))
