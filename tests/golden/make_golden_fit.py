"""
Golden values of Spline.least_squares.  Runs ONLY where the reference checkout is importable (see
make_golden.load_reference); the output, ``least_squares.npz``, holds per case the inputs, the knots and coefficients
the reference's ``Spline.least_squares`` returned, and two recorded numbers:

    kappa        product over the variables of cond_2(A) of the (final) collocation matrices
    ref_spread   largest difference, relative to max |coef|, between the reference's coefficients and an independent
                 NumPy solve of the same per-variable systems (Householder QR; a QR null-space step for fixEnds;
                 the pseudo-inverse for the rank-deficient case)

Tolerance cases also record ``gap``: over all iterations, the smallest relative distance between the largest row norm
and the second largest, and between the largest and the threshold.  A case with a gap under 1e-6 is refused: its knots
would be decided by rounding.

    python tests/golden/make_golden_fit.py

Keys: ``<case>/u<iv>``, ``<case>/data``, ``<case>/order``, ``<case>/args`` (compression, tolerance or nan, fixEnds),
``<case>/knots_in<iv>`` (explicit knots), ``<case>/knots<iv>``, ``<case>/coefs``, ``<case>/kappa``,
``<case>/ref_spread``, ``<case>/gap``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import load_reference  # noqa: E402
import fit_ref  # noqa: E402


def franke(x, y):
    return (0.75 * np.exp(-((9 * x - 2) ** 2 + (9 * y - 2) ** 2) / 4) + 0.75 * np.exp(-((9 * x + 1) ** 2) / 49 - (9 * y + 1) / 10)
            + 0.5 * np.exp(-((9 * x - 7) ** 2 + (9 * y - 3) ** 2) / 4) - 0.2 * np.exp(-((9 * x - 4) ** 2 + (9 * y - 7) ** 2)))


def jittered(rng, n, lo=0.0, hi=1.0, amount=0.3):
    u = np.linspace(lo, hi, n)
    u[1:-1] += (rng.random(n - 2) - 0.5) * amount * (hi - lo) / (n - 1)
    return u


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    u = np.sort(rng.random(2000) * 3.0 - 1.0)
    out["curve2000"] = dict(u=[u], data=np.stack([np.sin(3 * u), np.cos(2 * u) * u, np.exp(-u * u)]) + 0.01 * rng.standard_normal((3, 2000)),
                            compression=0.9)
    us = [jittered(rng, 200), jittered(rng, 150, -1.0, 2.0)]
    surf = (franke(us[0][:, None], (us[1][None, :] + 1.0) / 3.0) + 0.005 * rng.standard_normal((200, 150)))[None]
    out["surface_o43"] = dict(u=us, data=surf, order=(4, 3), compression=0.8)
    out["surface_o65"] = dict(u=us, data=surf, order=(6, 5), compression=0.5)
    ui = [jittered(rng, 40), jittered(rng, 30)]
    out["interpolation"] = dict(u=ui, data=np.stack([franke(ui[0][:, None], ui[1][None, :]), np.sin(4 * ui[0])[:, None] * ui[1][None, :]]),
                                compression=0.0)
    # Hermite: a repeated parameter = the next derivative of x(u) = (sin 2u, u^3 - u)
    base = np.linspace(0.0, 2.0, 41)
    reps = np.ones(41, int)
    reps[[0, 13, 40]] = 2
    reps[[7, 29]] = 3
    uh = np.repeat(base, reps)
    d = fit_ref.derivative_orders(uh)
    f0 = [np.sin(2 * uh), 2 * np.cos(2 * uh), -4 * np.sin(2 * uh)]
    f1 = [uh ** 3 - uh, 3 * uh ** 2 - 1, 6 * uh]
    out["hermite"] = dict(u=[uh], data=np.stack([np.choose(d, f0), np.choose(d, f1)]), order=(5,), compression=0.4)
    ue = np.linspace(0.0, 1.0, 41)
    out["knots_curve"] = dict(u=[ue], data=np.stack([np.cos(5 * ue), ue ** 2])[:, :],
                              order=(4,), knots=[np.array([0, 0, 0, 0, 0.2, 0.4, 0.4, 0.75, 1, 1, 1, 1.0])])
    ue2 = [np.linspace(-1.0, 1.0, 25), np.linspace(0.0, 2.0, 31)]
    out["knots_surface"] = dict(u=ue2, data=np.stack([np.outer(np.sin(2 * ue2[0]), np.cos(ue2[1])), np.outer(ue2[0], ue2[1] ** 2)]),
                                order=(3, 4), knots=[np.array([-1, -1, -1, -0.3, 0.1, 0.6, 1, 1, 1.0]),
                                                     np.array([0, 0, 0, 0, 0.5, 1.0, 1.1, 1.6, 2, 2, 2, 2.0])])
    u3 = [jittered(rng, 12), jittered(rng, 10), jittered(rng, 9)]
    g = np.meshgrid(*u3, indexing="ij")
    out["volume"] = dict(u=u3, data=np.stack([np.sin(2 * g[0]) * g[1] + g[2] ** 2, np.exp(-g[0] * g[1]) * np.cos(3 * g[2])]),
                         order=(3, 4, 3), compression=0.4)
    u32 = [jittered(rng, 64), jittered(rng, 48)]
    out["float32"] = dict(u=u32, data=(franke(u32[0][:, None], u32[1][None, :])[None] + 0.01 * rng.standard_normal((1, 64, 48))).astype(np.float32),
                          order=(4, 4), compression=0.7)
    uf = np.sort(rng.random(80))
    out["fixends_curve"] = dict(u=[uf], data=np.stack([np.sin(5 * uf), uf * np.cos(3 * uf)]) + 0.02 * rng.standard_normal((2, 80)),
                                compression=0.8, fixEnds=True)
    uf2 = [jittered(rng, 30), jittered(rng, 26)]
    out["fixends_surface"] = dict(u=uf2, data=franke(uf2[0][:, None], uf2[1][None, :])[None] + 0.01 * rng.standard_normal((1, 30, 26)),
                                  order=(4, 3), compression=0.6, fixEnds=True)
    # no parameter value inside [0.4, 0.6]: the B-spline that lives there has no data (Schoenberg-Whitney violated)
    ud = np.concatenate((np.linspace(0.0, 0.38, 20), np.linspace(0.62, 1.0, 20)))
    out["deficient"] = dict(u=[ud], data=np.stack([np.sin(6 * ud), ud])[:, :], order=(3,),
                            knots=[np.array([0, 0, 0, 0.2, 0.42, 0.47, 0.53, 0.58, 0.8, 1, 1, 1.0])])
    ut = [np.linspace(0.0, 1.0, 101), np.linspace(0.0, 1.0, 101)]
    out["tolerance_franke"] = dict(u=ut, data=franke(ut[0][:, None], ut[1][None, :])[None], tolerance=1.0e-4)
    uj = [jittered(rng, 80), jittered(rng, 61)]
    out["tolerance_jittered"] = dict(u=uj, data=franke(uj[0][:, None], uj[1][None, :])[None], order=(3, 5), tolerance=3.0e-4)
    return out


def independent_solve(A, b, fixed):
    if fixed:
        C, dvals = A[fixed], b[fixed]
        Af, bf = np.delete(A, fixed, 0), np.delete(b, fixed, 0)
        Q, R = np.linalg.qr(C.T, mode="complete")
        m = len(fixed)
        y = np.linalg.solve(R[:m].T, dvals)
        x1 = Q[:, :m] @ y
        N = Q[:, m:]
        return x1 + N @ fit_ref.qr_solve(Af @ N, bf - Af @ x1)
    if np.linalg.matrix_rank(A) < A.shape[1]:
        return np.linalg.pinv(A) @ b
    return fit_ref.qr_solve(A, b)


def main():
    bspy = load_reference()

    def ref_matrix(knots, order, u):
        A = np.zeros((len(u), len(knots) - order))
        d = fit_ref.derivative_orders(u)
        ix = None
        for r in range(len(u)):
            if d[r] == 0:
                ix = None
            ix, row = bspy.Spline.bspline_values(ix, knots, order, u[r], int(d[r]))
            A[r, ix - order:ix] = row
        return A

    out = {}
    for name, c in cases().items():
        u, data = c["u"], c["data"]
        order = c.get("order")
        kw = dict(compression=c.get("compression", 0.0), tolerance=c.get("tolerance"), fixEnds=c.get("fixEnds", False))
        s = bspy.Spline.least_squares(u if len(u) > 1 else u[0], data.astype(np.float64), order, c.get("knots"), **kw)
        order = list(s.order)
        coefs = np.asarray(s.coefs, np.float64)
        # the same per-variable systems, solved independently
        kappa, cur = 1.0, data.astype(np.float64)
        for iv in range(len(u)):
            A = ref_matrix(s.knots[iv], order[iv], u[iv])
            kappa *= np.linalg.cond(A)
            fixed = [r for r in range(len(u[iv])) if u[iv][r] in (u[iv][0], u[iv][-1])] if kw["fixEnds"] else []
            b = np.moveaxis(cur, iv + 1, 0)
            tail = b.shape[1:]
            x = independent_solve(A, b.reshape(len(u[iv]), -1), fixed)
            cur = np.moveaxis(x.reshape((A.shape[1],) + tail), 0, iv + 1)
        spread = float(np.abs(cur - coefs).max() / np.abs(coefs).max())
        gap = np.nan
        if kw["tolerance"] is not None:
            trace = []
            k2, c2 = fit_ref.fit(u, data, order, tolerance=kw["tolerance"], matrix=ref_matrix, trace=trace)
            assert all(np.array_equal(a, b) for a, b in zip(k2, s.knots)), f"{name}: restated loop found other knots"
            limit = kw["tolerance"] / len(u)
            gap = np.inf
            for norms in trace:
                top = np.sort(norms)[::-1]
                gap = min(gap, abs(top[0] - limit) / limit)
                if top[0] > limit:
                    gap = min(gap, (top[0] - top[1]) / top[0])
            assert gap >= 1e-6, f"{name}: arg-max decided by rounding (gap {gap:.1e})"
            print(f"  {len(trace)} solves, coefficient difference of the restated loop {np.abs(c2 - coefs).max():.1e}")
        print(f"{name}: nCoef {s.nCoef} kappa {kappa:.3e} ref_spread {spread:.3e} gap {gap:.2e}", flush=True)
        for iv in range(len(u)):
            out[f"{name}/u{iv}"] = np.asarray(u[iv], np.float64)
            out[f"{name}/knots{iv}"] = np.asarray(s.knots[iv], np.float64)
            if c.get("knots") is not None:
                out[f"{name}/knots_in{iv}"] = np.asarray(c["knots"][iv], np.float64)
        out[f"{name}/data"] = data
        out[f"{name}/order"] = np.array(order, np.int32)
        out[f"{name}/args"] = np.array([kw["compression"], np.nan if kw["tolerance"] is None else kw["tolerance"], float(kw["fixEnds"])])
        out[f"{name}/coefs"] = coefs
        out[f"{name}/kappa"] = np.float64(kappa)
        out[f"{name}/ref_spread"] = np.float64(spread)
        out[f"{name}/gap"] = np.float64(gap)
    path = os.path.join(HERE, "least_squares.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
