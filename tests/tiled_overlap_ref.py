"""Overlapped tiling, restated one output pixel at a time (include/srcfd.h, "overlapping tiles with blended seams").  Written from
the definition and independent of sr-for-cfd_amd/pipeline.py: scalar numpy float32 arithmetic, no strips, no shared helpers.  The
tests hold the host function to this and the device path to the host function.

`variant` builds the three wrong readings the tests must tell from the right one: "y_first" (blend along y before x), "flipped"
(w exchanged with 1 - w) and "shifted" (the zone one row / column late)."""
import numpy as np

F = np.float32


def pair(overlap):
    return (int(overlap[0]), int(overlap[1])) if isinstance(overlap, (tuple, list)) else (int(overlap), int(overlap))


def ramp(O):
    """w[j] = float32((j + 0.5) / O): the division in float64, rounded once."""
    return [F((j + 0.5) / float(O)) for j in range(O)]


def axis_source(R, T, S, O, shift=0):
    """(t0, r0, t1, r1, j): row R of an axis of T tiles, fine stride S, fine overlap O.  t0 is None where the row has one source."""
    t1 = min(R // S, T - 1)
    r1 = R - t1 * S
    if t1 >= 1 and shift <= r1 < O + shift and r1 + S < S + O:
        return t1 - 1, r1 + S, t1, r1, r1 - shift
    return None, None, t1, r1, None


def blend(a, b, w):
    """a + w * (b - a): three float32 operations, each rounded."""
    with np.errstate(all="ignore"):
        return F(F(a) + F(F(w) * F(F(b) - F(a))))


def cut(field, lr, overlap):
    """The tile samples (n, lr, lr, 1) of a (TY*(lr-oy)+oy, TX*(lr-ox)+ox, C) field, s = (ty*TX + tx)*C + c."""
    oy, ox = pair(overlap)
    H, W, C = field.shape
    ly, lx = lr - oy, lr - ox
    TY, TX = (H - oy) // ly, (W - ox) // lx
    assert TY * ly + oy == H and TX * lx + ox == W
    x = np.empty((TY * TX * C, lr, lr, 1), F)
    for ty in range(TY):
        for tx in range(TX):
            for c in range(C):
                for r in range(lr):
                    for col in range(lr):
                        x[(ty * TX + tx) * C + c, r, col, 0] = field[ty * ly + r, tx * lx + col, c]
    return x


def stitch(y, TY, TX, C, lh, lw, overlap, variant=None):
    """y (n, hh, hw[, 1]) planar samples -> (TY*Sy + Oy, TX*Sx + Ox, C), per pixel."""
    oy, ox = pair(overlap)
    y = np.asarray(y, F).reshape(TY * TX * C, y.shape[1], y.shape[2])
    hh, hw = y.shape[1], y.shape[2]
    assert hh % lh == 0 and hw % lw == 0 and 0 <= 2 * oy <= lh and 0 <= 2 * ox <= lw
    sy, sx = hh // lh, hw // lw
    Sy, Oy, Sx, Ox = (lh - oy) * sy, oy * sy, (lw - ox) * sx, ox * sx
    wy, wx = ramp(Oy), ramp(Ox)
    if variant == "flipped":
        wy, wx = [F(1) - w for w in wy], [F(1) - w for w in wx]
    shift = 1 if variant == "shifted" else 0
    out = np.empty((TY * Sy + Oy, TX * Sx + Ox, C), F)

    def val(ty, tx, c, r, col):
        return y[(ty * TX + tx) * C + c, r, col]

    for R in range(out.shape[0]):
        ty0, ry0, ty1, ry1, jy = axis_source(R, TY, Sy, Oy, shift)
        for X in range(out.shape[1]):
            tx0, cx0, tx1, cx1, jx = axis_source(X, TX, Sx, Ox, shift)
            for c in range(C):
                if variant == "y_first":
                    def along_y(tx, col):
                        b = val(ty1, tx, c, ry1, col)
                        return b if ty0 is None else blend(val(ty0, tx, c, ry0, col), b, wy[jy])
                    right = along_y(tx1, cx1)
                    out[R, X, c] = right if tx0 is None else blend(along_y(tx0, cx0), right, wx[jx])
                    continue

                def along_x(ty, r):
                    b = val(ty, tx1, c, r, cx1)
                    return b if tx0 is None else blend(val(ty, tx0, c, r, cx0), b, wx[jx])
                bottom = along_x(ty1, ry1)
                out[R, X, c] = bottom if ty0 is None else blend(along_x(ty0, ry0), bottom, wy[jy])
    return out


def zones(TY, TX, lh, lw, hh, hw, overlap):
    """Boolean (H, W) masks: rows blended along y, columns blended along x."""
    oy, ox = pair(overlap)
    sy, sx = hh // lh, hw // lw
    Sy, Oy, Sx, Ox = (lh - oy) * sy, oy * sy, (lw - ox) * sx, ox * sx
    H, W = TY * Sy + Oy, TX * Sx + Ox
    zy = np.array([axis_source(R, TY, Sy, Oy)[0] is not None for R in range(H)])
    zx = np.array([axis_source(X, TX, Sx, Ox)[0] is not None for X in range(W)])
    return np.broadcast_to(zy[:, None], (H, W)), np.broadcast_to(zx[None, :], (H, W))
