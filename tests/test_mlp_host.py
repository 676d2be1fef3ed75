"""Host side of the MLP maps (no GPU): rom_mlp_layout and its limits, the NumPy specification of the loss / gradient kernel
against the 80-bit truth of tests/mlp_truth.py (which central differences pin), the NumPy specification of the optimiser, the
initial weights, and the conditions on the fixed cases that tests/test_gpu_mlp.py relies on."""
import ctypes as C

import numpy as np
import pytest

from conftest import observed
import mlp_truth as mt

LD = mt.LD
LAYOUT_CASES = [(4, [20, 20], 77), (16, [64, 64], 16), (1, [1], 1), (64, [64], 1)]
#                m   hidden            q
INVALID = [(0,  [20],             1),      # m = 0
           (65, [20],             1),      # m = 65
           (4,  [65],             1),      # a width of 65
           (4,  [20],             129),    # q = 129
           (4,  [8, 8, 8, 8],     1),      # four hidden layers
           (64, [64, 64],         128)]    # 64 x 64 + 64 x 64 + 64 x 128 = 16384 padded weights: over the budget


def _scaled(case, held_out=False):
    """the case's weights and its scaled training rows (with held_out: every row, the held-out block included)"""
    cid, m, hidden, q, M, activation, gain, alpha, seed = case
    X, Y, w, sizes = mt.case_data(case)
    c, h, mean, scale = mt.scalings(X[:M], Y[:M])
    rows = len(X) if held_out else M
    return w, sizes, activation, mt.scale_inputs(X[:rows], c, h), mt.scale_targets(Y[:rows], mean, scale), alpha


@pytest.mark.parametrize("m,hidden,q", LAYOUT_CASES)
def test_layout_counts(m, hidden, q):
    from romhighcontrast_amd import _ffi
    lay = _ffi.mlp_layout(m, hidden, q)
    sizes = [m] + hidden + [q]
    P, wo, bo = mt.count(sizes)
    assert lay["P"] == P and lay["w_offsets"] == wo and lay["b_offsets"] == bo and lay["sizes"] == sizes
    pad = [(n + 15) // 16 * 16 for n in sizes]
    assert lay["padded_weights"] == sum(a * b for a, b in zip(pad, pad[1:])) <= 9216
    assert lay["lds_predict"] <= lay["lds_eval"] <= 160 * 1024 and lay["layers"] == len(hidden) + 1
    assert lay["n_weights"] == sum(a * b for a, b in zip(sizes, sizes[1:]))


@pytest.mark.parametrize("m,hidden,q", INVALID)
def test_layout_limits(m, hidden, q):
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.nonlinear import MLPMap
    lib = _ffi.load_library()
    hid = np.asarray(hidden, dtype=np.int32)
    out, off = np.zeros(8, dtype=np.int64), np.zeros(16, dtype=np.int64)
    assert lib.rom_mlp_layout(m, len(hid), hid.ctypes.data, q, out.ctypes.data, off.ctypes.data) == _ffi.ROM_ERR_INVALID
    assert "rom_mlp_layout" in _ffi.last_error()
    with pytest.raises(ValueError):
        _ffi.mlp_layout(m, hidden, q)
    # the map refuses the shape before any device call (there may be no device here)
    with pytest.raises(ValueError):
        MLPMap(hidden_layer_sizes=hidden).fit(np.zeros((6, m)), np.zeros((6, q)))


def test_two_flagship_shapes_and_the_widest_output_are_inside_the_limits():
    from romhighcontrast_amd import _ffi
    for m, hidden, q in ((4, [20, 20], 77), (16, [64, 64], 16), (1, [64], 128), (64, [16], 1), (16, [17, 33, 15], 17)):
        assert _ffi.mlp_layout(m, hidden, q)["lds_eval"] <= 160 * 1024
    # inside the weight budget, but the slab and the weights do not fit the LDS of one workgroup: the second rule
    with pytest.raises(ValueError, match="LDS"):
        _ffi.mlp_layout(48, [32, 64, 16], 128)


def test_prototypes_and_estimator_limits():
    from romhighcontrast_amd import _ffi
    from romhighcontrast_amd.lib.Estimators import EstimatorNN
    lib = _ffi.load_library()
    for name in ("rom_mlp_layout", "rom_mlp_fit", "rom_mlp_loss_grad", "rom_mlp_predict", "rom_mlp_query", "rom_mlp_download",
                 "rom_mlp_destroy"):
        assert name in _ffi.PROTOTYPES and hasattr(lib, name), name
    assert len(_ffi.PROTOTYPES["rom_mlp_fit"][1]) == 21 and len(_ffi.PROTOTYPES["rom_mlp_predict"][1]) == 12
    assert _ffi.PROTOTYPES["rom_mlp_predict"] == _ffi.PROTOTYPES["rom_poly_predict"]
    est = EstimatorNN(np.ones((5, 2)), (8, 8), max_iter=3)
    assert len(est.tree) == 2 and est.tree[0].hidden_layer_sizes == (8, 8) and est.tree[0].max_iter == 3
    with pytest.raises(ValueError):
        EstimatorNN(np.ones((65, 2)), (8,))
    with pytest.raises(ValueError):
        EstimatorNN(np.ones((5, 2)), (8, 8, 8, 8))


@pytest.mark.parametrize("case", mt.CASES, ids=[c[0] for c in mt.CASES])
def test_numpy_specification_against_the_truth(case):
    """mlp_loss_grad_host in fp64 within the bound of the 80-bit truth; the same function in long double agrees with the truth
    (an independent implementation) to long-double rounding."""
    from romhighcontrast_amd.nonlinear import mlp_loss_grad_host
    w, sizes, activation, T, Ys, alpha = _scaled(case)
    L, g = mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha)
    assert g.dtype == np.float64 and g.shape == (mt.count(sizes)[0],)
    rl, rg = mt.ratios(L, g, w, sizes, activation, T, Ys, alpha)
    observed(f"mlp {case[0]}: NumPy fp64 |loss - 80-bit| / ((M + sum K + 32) eps L_abs)", rl, 1.0)
    observed(f"mlp {case[0]}: NumPy fp64 max |grad - 80-bit| / ((M + sum K + 32) eps G_abs)", rg, 1.0)
    Ll, gl = mlp_loss_grad_host(w, sizes, activation, T, Ys, alpha, dtype=LD)
    assert gl.dtype == np.dtype(LD)
    eps_ld = float(np.finfo(LD).eps)
    rl, rg = mt.ratios(Ll, gl, w, sizes, activation, T, Ys, alpha)
    # (the same bound with the long-double eps in place of 2^-53: ratio * 2^-53 / eps_ld <= 1)
    assert rl * mt.EPS / eps_ld <= 1.0 and rg * mt.EPS / eps_ld <= 1.0, (rl, rg)
    # a gradient that forgets one row is far outside the bound: the bound is not vacuous
    if len(T) > 1:
        L1, g1 = mlp_loss_grad_host(w, sizes, activation, T[:-1], Ys[:-1], alpha)
        assert mt.ratios(L1, g1 * (len(T) - 1) / len(T), w, sizes, activation, T, Ys, alpha)[1] > 1e4


@pytest.mark.parametrize("case", [c for c in mt.CASES if c[5] != "relu"], ids=[c[0] for c in mt.CASES if c[5] != "relu"])
def test_central_differences_pin_the_truth(case):
    """(L(w + d e_p) - L(w - d e_p)) / 2d in long double, d = 1e-6, on 20 random entries.  Its error is d^2 |L'''| / 6 + eps_ld L / d
    = 1e-12 |L'''| + 1e-13 L: with third derivatives up to a few hundred (weights at 6 x Glorot) that is below 1e-9 (1 + |g_p|)."""
    w, sizes, activation, T, Ys, alpha = _scaled(case)
    _, g = mt.loss_grad(w, sizes, activation, T, Ys, alpha)
    rng = np.random.default_rng(5)
    d = LD(1e-6)
    worst = 0.0
    for p in rng.choice(len(w), size=min(20, len(w)), replace=False):
        wp, wm = w.astype(LD), w.astype(LD)
        wp[p] += d
        wm[p] -= d
        fd = (mt.loss_grad(wp, sizes, activation, T, Ys, alpha)[0] - mt.loss_grad(wm, sizes, activation, T, Ys, alpha)[0]) / (2 * d)
        worst = max(worst, float(abs(fd - g[p]) / (1 + abs(g[p]))))
    observed(f"mlp {case[0]}: |central difference - truth gradient| / (1 + |g|) / 1e-9", worst / 1e-9, 1.0)


@pytest.mark.parametrize("case", [c for c in mt.CASES if c[5] == "relu"], ids=[c[0] for c in mt.CASES if c[5] == "relu"])
def test_relu_cases_stay_clear_of_the_kink(case):
    """the condition on the fixed seeds: every 80-bit hidden pre-activation has |z| > 2^-30 (asserted inside forward), on the
    training rows and on the held-out block"""
    w, sizes, activation, T, Ys, alpha = _scaled(case, held_out=True)
    mt.forward(w, sizes, activation, T)


def _opt_problem(case):
    from romhighcontrast_amd.nonlinear import MLPMap
    cid, m, hidden, q, M, activation, seed = case
    X, Y, sizes = mt.opt_data(case)
    c, h, mean, scale = mt.scalings(X, Y)
    return MLPMap.initial_weights(sizes, activation, seed), sizes, activation, mt.scale_inputs(X, c, h), mt.scale_targets(Y, mean, scale)


@pytest.mark.parametrize("case", mt.OPT_CASES, ids=[c[0] for c in mt.OPT_CASES])
def test_optimiser_specification(case):
    from romhighcontrast_amd.nonlinear import mlp_fit_host
    w0, sizes, activation, T, Ys = _opt_problem(case)
    args = (sizes, activation, T, Ys, mt.OPT_ALPHA)
    zero = mlp_fit_host(w0, *args, 0, mt.OPT_TOL, mt.OPT_MEMORY)
    assert zero["iterations"] == 0 and zero["evaluations"] == 1 and zero["stop"] == 2 and zero["trials"] == []
    assert np.array_equal(zero["w"].view(np.uint64), w0.view(np.uint64)), "max_iter = 0 returns w0 bit for bit"
    # the fp64 and the long-double run take the same trial counts on the cases the GPU test uses
    for it in (1, 2, 3):
        a = mlp_fit_host(w0, *args, it, mt.OPT_TOL, mt.OPT_MEMORY)
        b = mlp_fit_host(w0, *args, it, mt.OPT_TOL, mt.OPT_MEMORY, dtype=LD)
        assert a["trials"] == b["trials"] and a["iterations"] == b["iterations"] == it and a["stop"] == b["stop"] == 2, (a["trials"], b["trials"])
        assert a["evaluations"] == 1 + sum(a["trials"]) and b["w"].dtype == np.dtype(LD)
        print(f"{case[0]} max_iter = {it}: trials {a['trials']}, max |w fp64 - w long double| = {float(np.abs(a['w'] - b['w']).max()):.3e}")
    full = mlp_fit_host(w0, *args, 60, mt.OPT_TOL, mt.OPT_MEMORY)
    assert np.all(np.diff(full["loss_curve"]) <= 0) and len(full["loss_curve"]) == full["iterations"] + 1
    assert full["loss"] == full["loss_curve"][-1] < 0.2 * full["loss_curve"][0]
    loose = mlp_fit_host(w0, *args, 100, 1e-1, mt.OPT_MEMORY)
    assert loose["stop"] == 0 and loose["grad_inf"] <= 1e-1 and loose["iterations"] < 100


def test_line_search_failure_is_reachable():
    """relu kinks (2 -> 3 -> 2, 40 rows, tol = 0): after 72 iterations no trial of the line search decreases the loss"""
    from romhighcontrast_amd.nonlinear import MLPMap, mlp_fit_host
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, (40, 2))
    Y = mt.smooth_map(X, 2)
    c, h, mean, scale = mt.scalings(X, Y)
    sizes = [2, 3, 2]
    res = mlp_fit_host(MLPMap.initial_weights(sizes, "relu", 1), sizes, "relu", mt.scale_inputs(X, c, h), mt.scale_targets(Y, mean, scale),
                       1e-4, 20000, 0.0, 10)
    assert res["stop"] == 3 and res["trials"][-1] == 30 and res["iterations"] == len(res["trials"]) - 1
    assert np.all(np.diff(res["loss_curve"]) <= 0)


def test_initial_weights():
    from romhighcontrast_amd.nonlinear import MLPMap
    sizes = [4, 20, 20, 5]
    a, b = MLPMap.initial_weights(sizes, "tanh", 3), MLPMap.initial_weights(sizes, "tanh", 3)
    assert np.array_equal(a, b) and a.shape == (mt.count(sizes)[0],)
    assert not np.array_equal(a, MLPMap.initial_weights(sizes, "tanh", 4))
    Ws, bs = mt.split(a, sizes)
    for (k, n), W, bias in zip(zip(sizes[:-1], sizes[1:]), Ws, bs):
        bound = np.sqrt(6.0 / (k + n))
        assert W.shape == (n, k) and np.abs(W).max() <= bound and np.abs(bias).max() <= bound and np.abs(W).max() > 0.8 * bound
    lw = MLPMap.initial_weights(sizes, "logistic", 3)
    assert np.array_equal(lw, MLPMap.initial_weights(sizes, "sigmoid", 3)) and np.abs(lw).max() <= np.sqrt(2.0 / 24)
    # scikit-learn's draw: per layer W (fan_in, fan_out), then b, from RandomState(random_state)
    rng = np.random.RandomState(3)
    W0 = rng.uniform(-np.sqrt(6.0 / 24), np.sqrt(6.0 / 24), (4, 20))
    b0 = rng.uniform(-np.sqrt(6.0 / 24), np.sqrt(6.0 / 24), 20)
    assert np.array_equal(Ws[0], W0.T) and np.array_equal(bs[0], b0)
    m = MLPMap(activation="sigmoid")
    assert m.activation == "logistic" and m.steps[0][0] == "NN device" and m.steps[0][1] is m and m.hidden_layer_sizes == (20, 20)
    with pytest.raises(ValueError):
        MLPMap(activation="gelu")


def test_sensing_refuses_an_mlp():
    from romhighcontrast_amd.nonlinear import MLPMap, PolynomialSensing
    with pytest.raises(TypeError):
        PolynomialSensing(None, None, MLPMap())
