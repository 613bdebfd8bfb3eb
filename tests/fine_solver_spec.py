"""The fine-mesh solver's specification, restated in numpy (csrc/fine_solver.hip reproduces it bit for bit).

The outer loop and every expression are srcfd_coarse_solve's (csrc/coarse_solver.cpp), in the same operation order; numpy's
float64 element-wise operations round exactly as the device's do (-ffp-contract=off, correctly rounded division and sqrt).
What differs from the host solver, on purpose, is the inner sweep order, which has to be race-free on the device:
  momentum   Jacobi (every read from the previous iterate);
  pressure   red-black in place, colour (i + j) & 1, colour 0 first.
Sums of squares are reduced in the device's fixed order: per mesh row, thread t of 256 adds the row's values t, t + 256, ...
in order, then a halving tree; the row partials are summed the same way (`_sum256`).  The inner exit rule is the host's: at
least one sweep, stop when sqrt(sum R^2 / (nx ny)) < 1e-6, at most 1000 sweeps.

This file was written together with the kernels, so equal bits cannot show a mistake both share.  What pins it to something
independent is tests/test_fine_cross.py: this specification against the host solver itself on the cases of
tests/solver_cross.py -- dx != dy with nx > ny and nx < ny, QUICK and UPWIND on the cavity and on the backward-facing step,
rho != 1, relaxation factors, the step geometry and inlet rows, single lids, moving side walls, a channel with mixed boundary
types -- along trajectories from zero fields and at the fixed point, within the noise of the 1e-6 inner exit rule (velocities
to 2.3e-6, pressure to 9e-6; bounds 4 x the per-case measurement).  tests/test_gpu_fine_cross.py holds the device to the host
solver at the same bounds.
"""
from __future__ import annotations

import numpy as np

NT = 256
CAP = 1000


def _tree(a):
    """a (..., 256): lds[t] += lds[t + s] for s = 128 .. 1; returns lds[0]."""
    a = a.copy()
    s = NT // 2
    while s > 0:
        a[..., :s] = a[..., :s] + a[..., s:2 * s]
        s //= 2
    return a[..., 0]


def _thread_sums(vals):
    """vals (..., n) in thread order: thread t adds vals[t], vals[t + 256], ... starting from 0.0."""
    n = vals.shape[-1]
    q = max(1, -(-n // NT))
    pad = np.zeros(vals.shape[:-1] + (q * NT,))
    pad[..., :n] = vals
    pad = pad.reshape(vals.shape[:-1] + (q, NT))
    acc = np.zeros(vals.shape[:-1] + (NT,))
    for r in range(q):
        acc = acc + pad[..., r, :]
    return acc


def _sum256(vals):
    """block_sum(sum over a thread's strided elements) of the last axis."""
    return _tree(_thread_sums(vals))


class Spec:
    def __init__(self, nx, ny, lx, ly, Re, rho, dt, scheme, tol, bc_type, bc_value, bfs=None, relax=(0.5, 0.5, 0.2)):
        self.nx, self.ny = nx, ny
        self.dx, self.dy = lx / nx, ly / ny
        self.volp = self.dx * self.dy
        self.nu, self.rho, self.dt = 1.0 / Re, rho, dt
        self.quick = scheme == "QUICK"
        self.tol = [float(t) for t in tol]
        self.bc_type = np.asarray(bc_type, int).reshape(3, 4)
        self.bc_value = np.asarray(bc_value, float).reshape(3, 4)
        self.bfs = bfs                      # None or (step_height, h, Ub)
        self.relax = [float(r) for r in relax]
        self.Var = np.zeros((3, nx + 2, ny + 2))
        self.Old = np.zeros_like(self.Var)
        self.Ff = np.zeros((4, nx + 2, ny + 2))
        self.count = 0
        self.converged = False
        self.rms = np.zeros(3)
        self.sweeps = []                    # per outer iteration: [u, v, p] inner sweeps
        self.history = []
        I, J = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), indexing="ij")
        self._I, self._J = I, J
        self._colour_idx = {}
        # flat indices of Grid::vw's far reads (wrap per axis when negative, run on in flat memory, clamp at the end)
        self._far = {}
        sx, sy, size = (nx + 2) * (ny + 2), ny + 2, 3 * (nx + 2) * (ny + 2)
        for k in (0, 1):
            for name, (di, dj) in {"e": (2, 0), "w": (-2, 0), "n": (0, 2), "s": (0, -2)}.items():
                ii, jj = I + di, J + dj
                ii = np.where(ii < 0, ii + nx + 2, ii)
                jj = np.where(jj < 0, jj + ny + 2, jj)
                self._far[k, name] = np.minimum(k * sx + ii * sy + jj, size - 1)

    # ------------------------------------------------------------------ pieces
    def bc(self, k):
        V, t, val, nx, ny = self.Var, self.bc_type[k], self.bc_value[k], self.nx, self.ny
        V[k, 0, 1:ny + 1] = 2 * val[0] - V[k, 1, 1:ny + 1] if t[0] == 0 else V[k, 1, 1:ny + 1]
        V[k, nx + 1, 1:ny + 1] = 2 * val[1] - V[k, nx, 1:ny + 1] if t[1] == 0 else V[k, nx, 1:ny + 1]
        V[k, 1:nx + 1, ny + 1] = 2 * val[2] - V[k, 1:nx + 1, ny] if t[2] == 0 else V[k, 1:nx + 1, ny]
        V[k, 1:nx + 1, 0] = 2 * val[3] - V[k, 1:nx + 1, 1] if t[3] == 0 else V[k, 1:nx + 1, 1]
        if self.bfs is not None and k <= 1:
            step_h, h, Ub = self.bfs
            for j in range(1, ny + 1):
                y = (j - 0.5) * self.dy
                if y < step_h:
                    V[k, 0, j] = -V[k, 1, j]
                    continue
                if k == 1:
                    V[1, 0, j] = -V[1, 1, j]
                    continue
                yp = min(max(y - step_h, 0.0), h)
                u_in = 6.0 * Ub * (yp / h) * (1.0 - (yp / h))
                V[0, 0, j] = 2.0 * u_in - V[0, 1, j]
                V[1, 0, j] = -V[1, 1, j]

    def linear_interpolation(self):
        V, F, nx, ny = self.Var, self.Ff, self.nx, self.ny
        c = (slice(1, nx + 1), slice(1, ny + 1))
        F[0][c] = (V[0][c] + V[0, 2:nx + 2, 1:ny + 1]) * self.dy * 0.5
        F[1][c] = (V[1][c] + V[1, 1:nx + 1, 2:ny + 2]) * self.dx * 0.5
        F[2][c] = -(V[0][c] + V[0, 0:nx, 1:ny + 1]) * self.dy * 0.5
        F[3][c] = -(V[1][c] + V[1, 1:nx + 1, 0:ny]) * self.dx * 0.5

    def init(self, var=None):
        self.Var[:] = 0.0
        self.Old[:] = 0.0
        self.Ff[:] = 0.0
        if var is not None:
            self.Var[:, 1:-1, 1:-1] = np.asarray(var)[:, 1:-1, 1:-1]
        for k in range(3):
            self.bc(k)
        self.Old[:] = self.Var
        self.linear_interpolation()
        self.count, self.converged, self.sweeps, self.history = 0, False, [], []

    def _momentum_sweep(self, S, k):
        nx, ny = self.nx, self.ny
        c_ = (slice(1, nx + 1), slice(1, ny + 1))
        fe, fn, fw, fs = self.Ff[0][c_], self.Ff[1][c_], self.Ff[2][c_], self.Ff[3][c_]
        c = S[k][c_]
        ve, vw, vn, vs = S[k, 2:nx + 2, 1:ny + 1], S[k, 0:nx, 1:ny + 1], S[k, 1:nx + 1, 2:ny + 2], S[k, 1:nx + 1, 0:ny]
        z = np.zeros_like(c)
        if not self.quick:
            ue, uw, un, us = np.where(fe >= 0, c, ve), np.where(fw >= 0, c, vw), np.where(fn >= 0, c, vn), np.where(fs >= 0, c, vs)
            s = z
            for f in (fe, fw, fn, fs):
                s = np.where(f >= 0, s + f, s)
        else:
            flat = S.ravel()
            far = {n: flat[self._far[k, n]] for n in "ewns"}
            ue = np.where(fe >= 0, 0.75 * c + 0.375 * ve - 0.125 * vw, 0.75 * ve + 0.375 * c - 0.125 * far["e"])
            uw = np.where(fw >= 0, 0.75 * c + 0.375 * vw - 0.125 * ve, 0.75 * vw + 0.375 * c - 0.125 * far["w"])
            un = np.where(fn >= 0, 0.75 * c + 0.375 * vn - 0.125 * vs, 0.75 * vn + 0.375 * c - 0.125 * far["n"])
            us = np.where(fs >= 0, 0.75 * c + 0.375 * vs - 0.125 * vn, 0.75 * vs + 0.375 * c - 0.125 * far["s"])
            s = z
            for f in (fe, fw, fn, fs):
                s = s + np.where(f >= 0, 0.75 * f, 0.375 * f)
        Fc = ue * fe + uw * fw + un * fn + us * fs
        ap_c = s * self.volp
        Fd = self.volp * ((ve - 2.0 * c + vw) / (self.dx * self.dx) + (vn - 2.0 * c + vs) / (self.dy * self.dy))
        ap_d = -self.volp * (2.0 / (self.dx * self.dx) + 2.0 / (self.dy * self.dy))
        R = -(self.volp / self.dt * (c - self.Old[k][c_]) + Fc + (-self.nu) * Fd)
        ap = self.volp / self.dt + ap_c + (-self.nu) * ap_d
        D = S.copy()
        D[k][c_] = c + R / ap
        return D, _sum256(R * R)          # row partials

    def solve_momentum(self, k):
        S = self.Var.copy()
        n = 0
        for m in range(CAP):
            if m > 0:
                tot = _sum256(part)
                if np.sqrt(tot / (self.nx * self.ny)) < 1e-6:
                    break
            S, part = self._momentum_sweep(S, k)
            n = m + 1
        self.Var[k, 1:-1, 1:-1] = S[k, 1:-1, 1:-1]
        return n

    def solve_pressure(self):
        nx, ny = self.nx, self.ny
        c_ = (slice(1, nx + 1), slice(1, ny + 1))
        F = self.Ff
        rhs = self.rho / self.dt * (F[0][c_] + F[1][c_] + F[2][c_] + F[3][c_])
        ap_d = -self.volp * (2.0 / (self.dx * self.dx) + 2.0 / (self.dy * self.dy))
        P = self.Var[2]
        colour = (self._I + self._J) & 1
        n = 0
        parts = None
        for m in range(CAP):
            if m > 0:
                tot = _sum256(np.concatenate(parts))
                if np.sqrt(tot / (nx * ny)) < 1e-6:
                    break
            parts = []
            for col in (0, 1):
                p = P[c_]
                Fd = self.volp * ((P[2:nx + 2, 1:ny + 1] - 2.0 * p + P[0:nx, 1:ny + 1]) / (self.dx * self.dx) +
                                  (P[1:nx + 1, 2:ny + 2] - 2.0 * p + P[1:nx + 1, 0:ny]) / (self.dy * self.dy))
                R = rhs - Fd
                mask = colour == col
                P[c_] = np.where(mask, p + R / ap_d, p)
                parts.append(self._colour_partials(R * R, col))
            n = m + 1
        return n

    def _colour_partials(self, R2, col):
        """Row partials of one colour: row i's cells of that colour, in j order, thread t takes the t-th, (t+256)-th, ..."""
        idx = self._colour_idx.get(col)
        if idx is None:
            nx, ny = self.nx, self.ny
            L = (ny + 1) // 2
            idx = np.full((nx, L), nx * ny)            # padding points at an appended 0.0
            for r in range(nx):
                j0 = 1 if ((r + 2) & 1) == col else 2
                js = np.arange(j0, ny + 1, 2)
                idx[r, :len(js)] = r * ny + js - 1
            self._colour_idx[col] = idx
        return _sum256(np.append(R2.ravel(), 0.0)[idx])

    def under_relax(self, k, alpha):
        o = self.Old[k, 1:-1, 1:-1]
        self.Var[k, 1:-1, 1:-1] = o + alpha * (self.Var[k, 1:-1, 1:-1] - o)

    # ------------------------------------------------------------------ the outer loop (srcfd_coarse_solve's)
    def outer(self):
        nx, ny, dt, rho = self.nx, self.ny, self.dt, self.rho
        sw = []
        for k in (0, 1):
            sw.append(self.solve_momentum(k))
            if self.bfs is not None:
                self.under_relax(k, self.relax[k])
            self.bc(k)
        self.linear_interpolation()
        sw.append(self.solve_pressure())
        if self.bfs is not None:
            self.under_relax(2, self.relax[2])
        self.bc(2)
        V, c_ = self.Var, (slice(1, nx + 1), slice(1, ny + 1))
        P = V[2]
        V[0][c_] = V[0][c_] - dt / rho * (P[2:nx + 2, 1:ny + 1] - P[0:nx, 1:ny + 1]) / (2 * self.dx)
        V[1][c_] = V[1][c_] - dt / rho * (P[1:nx + 1, 2:ny + 2] - P[1:nx + 1, 0:ny]) / (2 * self.dy)
        res = []
        for k in range(3):
            d = V[k][c_] - self.Old[k][c_]
            res.append(_sum256(_sum256(d * d)[None, :])[0])
        self.bc(0)
        self.bc(1)
        p = P[c_]
        F = self.Ff
        F[0][c_] = F[0][c_] + -dt / rho * (P[2:nx + 2, 1:ny + 1] - p) * self.dy / self.dx
        F[1][c_] = F[1][c_] + -dt / rho * (P[1:nx + 1, 2:ny + 2] - p) * self.dx / self.dy
        F[2][c_] = F[2][c_] + -dt / rho * (P[0:nx, 1:ny + 1] - p) * self.dy / self.dx
        F[3][c_] = F[3][c_] + -dt / rho * (P[1:nx + 1, 0:ny] - p) * self.dx / self.dy
        rms = np.array([np.sqrt(r / (nx * ny)) / dt for r in res])
        self.rms = rms
        self.sweeps.append(sw)
        if not np.isfinite(rms).all():
            raise ValueError("Solver failed: NaN/Inf in residuals")
        self.converged = not any(rms[k] > self.tol[k] for k in range(3))
        if not self.converged:
            self.Old[:] = self.Var

    def run(self, n):
        for _ in range(n):
            if self.converged:
                break
            self.count += 1
            self.outer()
            if self.count % 100 == 0:
                self.history.append(self.rms.copy())
        return self.count


def from_problem(pb, scheme=None):
    """A Spec for the fields of a `_lib.CoarseProblem`."""
    bfs = (pb.step_height, pb.channel_height, pb.bulk_velocity) if pb.case_type == 1 else None
    return Spec(pb.nx, pb.ny, pb.lx, pb.ly, pb.reynolds, pb.rho, pb.dt, "QUICK" if pb.scheme == 0 else "UPWIND", list(pb.tolerance),
                [[pb.bc_type[k][s] for s in range(4)] for k in range(3)], [[pb.bc_value[k][s] for s in range(4)] for k in range(3)],
                bfs=bfs, relax=list(pb.relax))
