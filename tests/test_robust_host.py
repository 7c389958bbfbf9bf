"""
Robust ``fit_points`` on the CPU.  ``bsk_scatter_reweight_host`` and the scale estimate against the plain-float statement
(``scatter.reweight``, ``scatter.lower_median``) bit for bit; ``fit_batch(robust=...)`` on the data of tests/robust_cases.py:
Huber and Tukey bring every coefficient within the family's bar of the fit to the clean subset where the plain fit misses it
by more than 10^3 bars (checked here: that is what makes the test mean something); the fixed point, the scaling laws, what a
call without the new keywords returns, ``info`` and the errors.

Tukey takes the default 8 rounds: it gives a displaced point the weight 0.0 in the first round or two, and the fit is the
clean one from there.  Huber never removes a point, it bounds its pull by s = c sigma, so the fit's error is proportional to
sigma, and sigma falls by a constant factor a round (the smaller the fewer points are displaced; about 2 with 8 of 36
displaced) until it reaches the rounding noise of the clean residuals: from sigma ~ 40 to ~ 10^-15 that is log2(4 10^16) ~ 55
rounds, so the Huber cases run ROUNDS_HUBER = 64.
"""
import math

import numpy as np
import pytest

import robust_cases as rc
from robust_cases import bits
from bspy_amd import Spline, scatter

SIZES = (1, 2, 63, 64, 65, 257)
ROUNDS = {"huber": 64, "tukey": 8}
TINY = 5e-324


def reweight_inputs(N, s, seed):
    """Residuals around the threshold, weights with zeros, excluded points."""
    rng = np.random.default_rng(seed)
    r = rng.random(N) * 3.0 * s
    special = [0.0, s, math.nextafter(s, 0.0), math.nextafter(s, math.inf), 2.0 * s, s / 3.0]
    r[:min(N, len(special))] = special[:N]
    w0 = rng.random(N) + 0.5
    w0[rng.random(N) < 0.2] = 0.0
    key = rng.integers(0, 9, N)
    gone = rng.random(N) < 0.2
    if N > 6:
        gone[:6] = False
    key[gone] = -1
    r[gone] = np.nan
    return r, w0, key.astype(np.int64)


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("s", [1.0, 0.37, 3.0 * TINY, 2.0 ** -1030, 1e300])
@pytest.mark.parametrize("N", SIZES)
def test_reweight_host_is_the_statement(loss, s, N):
    r, w0, key = reweight_inputs(N, s, N)
    for weights in (w0, None):
        got = scatter.reweights(scatter.Host(), loss, s, r, weights, key)
        assert scatter.LAST_PATHS[-1] == "host scatter_reweight"
        want = [scatter.reweight(loss, float(r[i]), 1.0 if weights is None else float(weights[i]), int(key[i]), s) for i in range(N)]
        assert bits(got) == bits(np.array(want))
        assert bits(got[key < 0]) == bits((np.ones(N) if weights is None else weights)[key < 0])          # an excluded point keeps w0
    if N > 6:
        w = scatter.reweights(scatter.Host(), loss, s, r, None, key)
        assert w[0] == 1.0 and w[5] == (1.0 if loss == "huber" else w[5]) and w[3] < 1.0                   # r = 0, r < s, r just above s
        assert w[1] == (1.0 if loss == "huber" else 0.0) and w[2] <= 1.0                                    # r = s: Huber keeps, Tukey drops


@pytest.mark.parametrize("N", SIZES)
def test_scale_is_the_lower_median(N):
    rng = np.random.default_rng(N)
    for values in (rng.random(N), np.round(rng.random(N) * 4.0), np.zeros(N)):
        assert scatter.sigma(values) == scatter.SIGMA * scatter.lower_median([float(v) for v in values])
        assert scatter.lower_median([float(v) for v in values]) == np.sort(values)[(N - 1) // 2]
    assert scatter.sigma(np.zeros(0)) == 0.0


@pytest.mark.parametrize("name", ["curve", "surface"])
def test_the_plain_fit_misses_the_clean_fit(name):
    exact, bar = rc.clean(name)
    c = rc.case(name)
    assert (np.abs(exact - c["coefs"].reshape(exact.shape)) <= bar).all()         # the clean subset's fit is the known spline
    s, info = rc.fit(name, _path="host")
    assert (np.abs(s.coefs.reshape(exact.shape) - exact) / bar).max() > 1.0e3
    counts = {}
    for key, out in zip(scatter.assemble(scatter.Host(), scatter.Shape(c["order"], c["knots"]), c["uvw"], c["points"], None)["key"], c["displaced"]):
        total, bad = counts.get(int(key), (0, 0))
        counts[int(key)] = (total + 1, bad + int(out))
    assert all(4 * bad < total for total, bad in counts.values())


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("name", ["curve", "surface"])
def test_robust_fit_is_the_clean_fit(name, loss):
    exact, bar = rc.clean(name)
    c = rc.case(name)
    s, info = rc.fit(name, robust=loss, iterations=ROUNDS[loss], _path="host")
    ratio = (np.abs(s.coefs.reshape(exact.shape) - exact) / bar).max()
    print(f"robust {name} {loss}: coefficient error / bar {ratio:.3g}, last scale {info['scale'][-1]:.3g}, rounds {info['rounds']}")
    assert ratio <= 1.0
    assert len(info["scale"]) in (info["rounds"], info["rounds"] + 1) and len(info["objective"]) == info["rounds"] + 1
    assert info["rounds"] == ROUNDS[loss] or info["scale"][-1] == 0.0
    if loss == "tukey":
        assert bits(info["weights"][c["displaced"]]) == bits(np.zeros(int(c["displaced"].sum())))
    assert info["paths"].count("host scatter_reweight") == info["rounds"] and info["paths"].count("host scatter_solve") == info["rounds"] + 1
    again, more = rc.fit(name, weights=info["weights"], _path="host")          # the fixed point
    assert bits(again.coefs) == bits(s.coefs)
    assert bits(info["residual"]) == bits(more["residual"]) and info["rms"] == more["rms"] and info["max"] == more["max"]


@pytest.mark.parametrize("loss", ["huber", ("tukey", 3.0)])
def test_scaling_laws(loss):
    c = rc.case("curve")
    rng = np.random.default_rng(5)
    w0 = rng.random(c["uvw"].shape[1]) + 0.5
    w0[::9] = 0.0
    s, info = rc.fit("curve", weights=w0, robust=loss, iterations=3, _path="host")
    assert info["rounds"] == 3
    for k in (1, -1, 37, -37):
        t, more = rc.fit("curve", weights=np.ldexp(w0, k), robust=loss, iterations=3, _path="host")
        assert bits(t.coefs) == bits(s.coefs) and more["scale"] == info["scale"]
        assert bits(np.ldexp(more["weights"], -k)) == bits(info["weights"])
        t, more = scatter.fit_batch(c["uvw"], np.ldexp(c["points"], k), c["order"], c["knots"], weights=w0, robust=loss, iterations=3, _path="host")
        assert bits(np.ldexp(t.coefs, -k)) == bits(s.coefs) and bits(more["weights"]) == bits(info["weights"])
        assert [math.ldexp(x, -k) for x in more["scale"]] == info["scale"]
    # weights do not enter sigma: points of weight 0 do not count, the others count once
    counted = np.flatnonzero(w0 > 0.0)
    plain = rc.fit("curve", weights=w0, _path="host")[1]
    assert info["scale"][0] == scatter.sigma(plain["residual"][counted])


def test_iterations_and_info():
    first = None
    for iterations in (1, 2, 3):
        s, info = rc.fit("surface", robust="huber", iterations=iterations, smoothing=2.0 ** -20, _path="host")
        assert info["rounds"] == iterations == len(info["scale"]) and len(info["objective"]) == iterations + 1
        assert info["weights"].shape == (216,) and isinstance(info["weights"], np.ndarray)
        first = first or info
        assert info["scale"][0] == first["scale"][0] and info["objective"][0] == first["objective"][0]
    c = rc.case("surface")
    got = Spline.fit_points(c["uvw"], c["points"], c["order"], c["knots"], robust="huber", iterations=3, smoothing=2.0 ** -20, _path="host")
    assert bits(got.coefs) == bits(s.coefs)


def test_a_call_without_the_new_keywords_is_todays():
    s, info = rc.fit("surface", _path="host")
    assert info["paths"] == ["host scatter_key", "host scatter_gram", "host scatter_cell", "host scatter_fold", "host scatter_solve",
                             "host scatter_residual"]
    assert set(info) == {"status", "residual", "rms", "max", "empty", "objective", "uvw", "paths"}
    c = rc.case("surface")
    sh = scatter.Shape(c["order"], c["knots"])
    res = scatter.assemble(scatter.Host(), sh, c["uvw"], c["points"], None)
    assert bits(s.coefs.reshape(1, -1)) == bits(scatter.solve(sh, res["stencil"], res["rhs"]))


def test_an_exact_fit_ends_the_rounds():
    order, knots = (2,), [np.array([0, 0, 0.5, 1, 1.0])]
    u = np.array([0.0, 0.5, 1.0])
    s, info = scatter.fit_batch(u, np.array([[1.0, 2.0, 4.0]]), order, knots, robust="tukey", _path="host")
    assert info["scale"] == [0.0] and info["rounds"] == 0 and bits(info["weights"]) == bits(np.ones(3))


def test_tukey_can_take_all_weight_from_a_coefficient():
    c = rc.case("curve")
    points = c["points"].copy()
    first = c["uvw"][0] < 1.0 / 8.0                                            # the first cell: all points under coefficient 0
    points[:, first] += 1000.0
    keep = ~c["displaced"]
    with pytest.raises(ValueError, match="not positive definite: the pivot of row [0-3] .* smoothing > 0 makes it so"):
        scatter.fit_batch(c["uvw"][:, keep], points[:, keep], c["order"], c["knots"], robust="tukey", _path="host")


def test_errors():
    c = rc.case("curve")
    args = (c["uvw"], c["points"], c["order"], c["knots"])
    with pytest.raises(ValueError, match="robust must be None, 'huber', 'tukey' or .name, c., not 'cauchy'"):
        scatter.fit_batch(*args, robust="cauchy")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="the tuning constant c must be finite and > 0"):
            scatter.fit_batch(*args, robust=("huber", bad))
    with pytest.raises(ValueError, match="robust takes iterations >= 1"):
        scatter.fit_batch(*args, robust="huber", iterations=0)
    with pytest.raises(ValueError, match="solve must be None, 'device' or 'host'"):
        scatter.fit_batch(*args, solve="gpu")
    with pytest.raises(ValueError, match="solve='device': the device solve belongs to the device path"):
        scatter.fit_batch(*args, solve="device", _path="host")
    with pytest.raises(ValueError, match="solve='device': the device solve belongs to the device path"):
        scatter.fit_batch(*args, robust="huber", solve="device")             # 128 points: the host path
    scatter.fit_batch(*args, iterations=0, solve="host", _path="host")           # iterations without robust is not read
