"""
Robust ``fit_points`` on the GPU.  ``bsk_scatter_reweight`` against the plain-float statement bit for bit; then
``fit_batch(robust=...)`` on the data of tests/robust_cases.py: the host path, the device path with the host solve, the
device path with the device solve and CUDA tensors in give the same BYTES in coefficients, weights, scale, objective and
residuals for every ``iterations`` in 1 .. 3 and for the runs of tests/test_robust_host.py that reach the clean fit (so the
device results lie within the same bar); ``info["paths"]`` names every launch once per round; a call without the new
keywords returns the host path's bytes and today's list of launches.  The host results are computed once and shared.
"""
import functools

import numpy as np
import pytest

import robust_cases as rc
from robust_cases import bits
from test_robust_host import ROUNDS, SIZES, reweight_inputs
from bspy_amd import scatter

pytestmark = pytest.mark.gpu

ASSEMBLY = ["scatter_key", "scatter_gram", "scatter_cell", "scatter_fold"]


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("s", [0.37, 3.0 * 5e-324, 1e300])
@pytest.mark.parametrize("N", SIZES)
def test_reweight_device_is_the_statement(loss, s, N):
    import torch
    be = scatter.Device.current()
    r, w0, key = reweight_inputs(N, s, N)
    for weights in (w0, None):
        got = scatter.reweights(be, loss, s, torch.from_numpy(r).cuda(), None if weights is None else torch.from_numpy(weights).cuda(),
                                torch.from_numpy(key).cuda())
        assert scatter.LAST_PATHS[-1] == "scatter_reweight"
        want = [scatter.reweight(loss, float(r[i]), 1.0 if weights is None else float(weights[i]), int(key[i]), s) for i in range(N)]
        assert bits(got.cpu().numpy()) == bits(np.array(want))


@functools.lru_cache(maxsize=None)
def host(name, loss, iterations, smoothing):
    return rc.fit(name, robust=loss, iterations=iterations, smoothing=smoothing, _path="host")


def same(one, two, cuda=False):
    (s, info), (t, more) = one, two
    get = (lambda a: a.cpu().numpy()) if cuda else (lambda a: a)
    assert bits(s.coefs) == bits(t.coefs)
    assert bits(get(info["weights"])) == bits(more["weights"]) and bits(get(info["residual"])) == bits(more["residual"])
    assert info["scale"] == more["scale"] and info["objective"] == more["objective"] and info["rounds"] == more["rounds"]
    assert info["rms"] == more["rms"] and info["max"] == more["max"]


def launches(solve, rounds):
    one = ASSEMBLY + [solve, "scatter_residual"]
    return one + (["scatter_reweight"] + one) * rounds


@pytest.mark.parametrize("iterations", [1, 2, 3])
@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("name", ["curve", "surface"])
def test_paths_and_solves_give_the_same_bytes(name, loss, iterations):
    import torch
    want = host(name, loss, iterations, 2.0 ** -20)
    assert want[1]["rounds"] == iterations
    for solve, kernel in (("host", "host scatter_solve"), ("device", "scatter_solve")):
        got = rc.fit(name, robust=loss, iterations=iterations, smoothing=2.0 ** -20, solve=solve, _path="device")
        same(got, want)
        assert got[1]["paths"] == launches(kernel, iterations) and isinstance(got[1]["weights"], np.ndarray)
    c = rc.case(name)
    got = scatter.fit_batch(torch.from_numpy(c["uvw"]).cuda(), torch.from_numpy(c["points"]).cuda(), c["order"], c["knots"], robust=loss,
                            iterations=iterations, smoothing=2.0 ** -20, solve="device")
    same(got, want, cuda=True)
    assert got[1]["weights"].is_cuda and got[1]["paths"] == launches("scatter_solve", iterations)


@pytest.mark.parametrize("loss", ["huber", "tukey"])
@pytest.mark.parametrize("name", ["curve", "surface"])
def test_device_robust_fit_is_the_clean_fit(name, loss):
    exact, bar = rc.clean(name)
    c = rc.case(name)
    got = rc.fit(name, robust=loss, iterations=ROUNDS[loss], solve="device", _path="device")
    same(got, host(name, loss, ROUNDS[loss], 0.0))
    assert ((np.abs(got[0].coefs.reshape(exact.shape) - exact) / bar).max()) <= 1.0
    if loss == "tukey":
        assert bits(got[1]["weights"][c["displaced"]]) == bits(np.zeros(int(c["displaced"].sum())))
    again, _ = rc.fit(name, weights=got[1]["weights"], _path="device")         # the fixed point, through the host solve
    assert bits(again.coefs) == bits(got[0].coefs)


def test_solve_none_follows_the_threshold(monkeypatch):
    c = rc.case("surface")
    sh = scatter.Shape(c["order"], c["knots"])
    work = sh.n * scatter.half_bandwidth(sh) ** 2                              # n hb^2 of the 6 x 5 bicubic
    assert work == 30 * 18 * 18
    got = rc.fit("surface", robust="huber", iterations=1, _path="device")
    assert got[1]["paths"] == launches("host scatter_solve" if work < scatter.SOLVE_MIN_WORK else "scatter_solve", 1)
    monkeypatch.setattr(scatter, "SOLVE_MIN_WORK", work)
    got = rc.fit("surface", robust="huber", iterations=1, _path="device")
    assert got[1]["paths"] == launches("scatter_solve", 1)
    monkeypatch.setattr(scatter, "SOLVE_MIN_WORK", work + 1)
    assert rc.fit("surface", robust="huber", iterations=1, _path="device")[1]["paths"] == launches("host scatter_solve", 1)
    monkeypatch.setattr(scatter, "FORCE_SOLVE", "device")
    assert rc.fit("surface", robust="huber", iterations=1, _path="device")[1]["paths"] == launches("scatter_solve", 1)
    assert rc.fit("surface", _path="device")[1]["paths"] == launches("scatter_solve", 0)      # a plain fit may be pinned too


def test_a_call_without_the_new_keywords_is_todays():
    s, info = rc.fit("surface", _path="device")
    t, more = rc.fit("surface", _path="host")
    assert info["paths"] == launches("host scatter_solve", 0)
    assert set(info) == {"status", "residual", "rms", "max", "empty", "objective", "uvw", "paths"}
    assert bits(s.coefs) == bits(t.coefs) and bits(info["residual"]) == bits(more["residual"]) and info["objective"] == more["objective"]


def test_scaling_laws_on_the_device():
    c = rc.case("curve")
    w0 = np.random.default_rng(5).random(128) + 0.5
    w0[::9] = 0.0
    s, info = rc.fit("curve", weights=w0, robust="tukey", iterations=3, solve="device", _path="device")
    for k in (1, -37):
        t, more = rc.fit("curve", weights=np.ldexp(w0, k), robust="tukey", iterations=3, solve="device", _path="device")
        assert bits(t.coefs) == bits(s.coefs) and more["scale"] == info["scale"] and bits(np.ldexp(more["weights"], -k)) == bits(info["weights"])
        t, more = scatter.fit_batch(c["uvw"], np.ldexp(c["points"], k), c["order"], c["knots"], weights=w0, robust="tukey", iterations=3,
                                    solve="device", _path="device")
        assert bits(np.ldexp(t.coefs, -k)) == bits(s.coefs) and bits(more["weights"]) == bits(info["weights"])


def test_errors_on_the_device():
    c = rc.case("curve")
    five = np.vstack([c["points"], c["points"], c["points"][:1]])
    with pytest.raises(ValueError, match="device path covers orders 2 to 4 and nDep 1 to 4"):
        scatter.fit_batch(c["uvw"], five, c["order"], c["knots"], robust="huber", solve="device", _path="device")
    with pytest.raises(ValueError, match="solve='device': the device solve belongs to the device path"):
        scatter.fit_batch(c["uvw"], five, c["order"], c["knots"], robust="huber", solve="device")
    with pytest.raises(ValueError, match="not positive definite: the pivot of row [0-3] .* smoothing > 0 makes it so"):
        points = c["points"].copy()
        points[:, c["uvw"][0] < 1.0 / 8.0] += 1000.0
        keep = ~c["displaced"]
        scatter.fit_batch(c["uvw"][:, keep], points[:, keep], c["order"], c["knots"], robust="tukey", solve="device", _path="device")
