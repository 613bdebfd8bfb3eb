"""References for the direct pressure solve (csrc/poisson_direct.hip, `pressure="direct"`), in numpy and scipy.

`solve_pressure` of the specification (tests/fine_solver_spec.py) keeps the ghost ring of the pressure plane frozen for the whole
inner solve, so each inner solve is the Dirichlet problem
    volp (Dxx / dx^2 + Dyy / dy^2) p = g,     g = rhs - volp (ghost neighbours / dx^2 or dy^2)
on the nx x ny interior, with solution  p = Sx [ (Sx g Sy) / Lambda ] Sy,
    S_n[a][b] = sqrt(2 / (n + 1)) sin(pi (a + 1)(b + 1) / (n + 1)),   Lambda[a][b] = volp (lambda_x[a] / dx^2 + lambda_y[b] / dy^2),
    lambda[a] = -4 sin^2(pi (a + 1) / (2 (n + 1))).
Three subclasses of `Spec` override `solve_pressure` alone with three evaluations of that solution and return 1 sweep:
  DirectDST    scipy.fft.dstn(type=1, norm="ortho");
  DirectGEMM   the same formula with numpy matrix products, the form the device evaluates;
  DirectLU     np.linalg.solve on the dense Kronecker matrix (nx ny <= 1200): no transform, no eigenvalue formula.
The direct mode has no numpy twin with equal bits.  It is a third float64 evaluation of the formula and differs from the two
transform evaluations only in the order of its sums, so `bound` measures what that order is worth -- the distance of the two CPU
evaluations at the same checkpoint -- and allows the device 8 times that (room for the MFMA's 4-deep chunks against BLAS
blocking), with a floor of 64 ulp of the field's largest value.  The bound never sees the device's result.

`DirectDST` takes three perturbations (a class attribute each) for the sensitivity test: dx exchanged for dy in Lambda, a dropped
ghost term, lambda of n + 1.
"""
from __future__ import annotations

import numpy as np
import scipy.fft

import fine_solver_spec as spec

U = 2.0 ** -53
PI = np.arccos(np.longdouble(-1))       # np.pi is pi rounded to float64: 1.2e-16 off, which sin(pi m / (n + 1)) shows at large m
LU_MAX_CELLS = 1200


def eigenvalues(n, size=None):
    """lambda[a] = -4 sin^2(pi (a + 1) / (2 (size + 1))), a < n (size: n unless the sensitivity test says otherwise), float64."""
    size = n if size is None else size
    a = np.arange(1, n + 1, dtype=np.longdouble)
    return (-4 * np.sin(PI * a / (2 * (np.longdouble(size) + 1))) ** 2).astype(np.float64)


def basis(n):
    """S_n in float64, from numpy's long double; the integer (a + 1)(b + 1) is reduced by the period 2 (n + 1) first."""
    a = np.arange(1, n + 1, dtype=np.int64)
    m = (np.outer(a, a) % (2 * (n + 1))).astype(np.longdouble)
    return (np.sqrt(np.longdouble(2) / (n + 1)) * np.sin(PI * m / (n + 1))).astype(np.float64)


def condition_number(nx, ny, dx, dy):
    """kappa of the system from the closed-form eigenvalues (volp cancels)."""
    lam = np.abs(eigenvalues(nx)[:, None] / dx ** 2 + eigenvalues(ny)[None, :] / dy ** 2)
    return float(lam.max() / lam.min())


class _Direct(spec.Spec):
    swap_dx_dy = False       # sensitivity: dx for dy in Lambda
    drop_ghost = False       # sensitivity: the i = 1 ghost term is left out
    lambda_of_n_plus_1 = False

    def rhs_and_ghosts(self):
        """g (nx, ny): rhs less the frozen ghost neighbours' share of the stencil."""
        nx, ny = self.nx, self.ny
        c_ = (slice(1, nx + 1), slice(1, ny + 1))
        F, P = self.Ff, self.Var[2]
        rhs = self.rho / self.dt * (F[0][c_] + F[1][c_] + F[2][c_] + F[3][c_])
        ghost_x, ghost_y = np.zeros((nx, ny)), np.zeros((nx, ny))
        if not self.drop_ghost:
            ghost_x[0] = ghost_x[0] + P[0, 1:ny + 1]
        ghost_x[-1] = ghost_x[-1] + P[nx + 1, 1:ny + 1]
        ghost_y[:, 0] = ghost_y[:, 0] + P[1:nx + 1, 0]
        ghost_y[:, -1] = ghost_y[:, -1] + P[1:nx + 1, ny + 1]
        return rhs - (self.volp / (self.dx * self.dx) * ghost_x + self.volp / (self.dy * self.dy) * ghost_y)

    def Lambda(self):
        dx, dy = (self.dy, self.dx) if self.swap_dx_dy else (self.dx, self.dy)
        extra = 1 if self.lambda_of_n_plus_1 else 0
        lx, ly = eigenvalues(self.nx, self.nx + extra), eigenvalues(self.ny, self.ny + extra)
        return self.volp * (lx[:, None] / (dx * dx) + ly[None, :] / (dy * dy))

    def exact(self, g):
        raise NotImplementedError

    def solve_pressure(self):
        self.Var[2, 1:-1, 1:-1] = self.exact(self.rhs_and_ghosts())
        return 1


class DirectDST(_Direct):
    def exact(self, g):
        t = scipy.fft.dstn(g, type=1, norm="ortho") / self.Lambda()
        return scipy.fft.dstn(t, type=1, norm="ortho")


class DirectGEMM(_Direct):
    def exact(self, g):
        Sx, Sy = basis(self.nx), basis(self.ny)
        t = ((Sx @ g) @ Sy) / self.Lambda()
        return (Sx @ t) @ Sy


class DirectLU(_Direct):
    def exact(self, g):
        nx, ny = self.nx, self.ny
        if nx * ny > LU_MAX_CELLS:
            raise ValueError(f"DirectLU takes at most {LU_MAX_CELLS} cells, not {nx} x {ny}")
        D = lambda n: -2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
        A = self.volp * (np.kron(D(nx), np.eye(ny)) / (self.dx * self.dx) + np.kron(np.eye(nx), D(ny)) / (self.dy * self.dy))
        return np.linalg.solve(A, g.ravel()).reshape(nx, ny)


def from_problem(cls, pb):
    """`spec.from_problem` for one of the classes here."""
    bfs = (pb.step_height, pb.channel_height, pb.bulk_velocity) if pb.case_type == 1 else None
    return cls(pb.nx, pb.ny, pb.lx, pb.ly, pb.reynolds, pb.rho, pb.dt, "QUICK" if pb.scheme == 0 else "UPWIND", list(pb.tolerance),
               [[pb.bc_type[k][s] for s in range(4)] for k in range(3)], [[pb.bc_value[k][s] for s in range(4)] for k in range(3)],
               bfs=bfs, relax=list(pb.relax))


def distances(a, b):
    """max |a - b| of u, v and p over the whole (nx + 2, ny + 2) planes."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.array([d[k].max() for k in range(3)])


def bound(a, b):
    """Per field, what the device may differ from `a` (DirectDST's Var) by: 8 x max |a - b| with b DirectGEMM's Var at the same
    checkpoint, and at least 64 ulp of the field's largest value."""
    a, b = np.asarray(a), np.asarray(b)
    return np.maximum(8.0 * distances(a, b), 64.0 * U * np.array([np.abs(a[k]).max() for k in range(3)]))


def forward_bound(nx, ny, dx, dy):
    """The worst-case forward error of one solve in relative 2-norm: 16 max(nx, ny) u kappa."""
    return 16.0 * max(nx, ny) * U * condition_number(nx, ny, dx, dy)


def smooth_state(nx, ny, seed):
    """A seeded, smooth, non-zero state (the one of tests/test_gpu_fine_batch.py)."""
    rng = np.random.default_rng(seed)
    x = (np.arange(1, nx + 1) - 0.5) / nx
    y = (np.arange(1, ny + 1) - 0.5) / ny
    X, Y = np.meshgrid(x, y, indexing="ij")
    var = np.zeros((3, nx + 2, ny + 2))
    for k in range(3):
        a, b, c = rng.uniform(0.5, 1.5, 3)
        ph = rng.uniform(0, np.pi, 2)
        var[k, 1:-1, 1:-1] = 0.3 * a * np.sin(np.pi * (b * X) + ph[0]) * np.cos(np.pi * (c * Y) + ph[1]) + 0.05 * k
    return var
