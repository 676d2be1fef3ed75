"""The host truth of the device trees (tests/tree_truth.py) against scikit-learn, and the checker against mutations.

scikit-learn works on a float32 copy of X and refuses thresholds between values closer than FEATURE_THRESHOLD = 1e-7, so the
inputs here are exactly representable in float32 with all gaps > 1e-7.  With m = 1 there are no cross-input ties and the tree
is unique: exact parity.  With m > 1 scikit-learn draws the ties at random (random_state), so the truth's held-out RMSE must
lie within 10 % of the median of scikit-learn's over random_state 0 .. 19: twice the largest deviation from that median seen
when the band was set (4-5 %; tree: truth 0.825 against 0.855 .. 0.874; forests 0.647 .. 0.649 against 0.670 .. 0.681)."""
import numpy as np
import pytest

import tree_truth as tt

N_TEST = 100


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _distinct_f32(rng, n, scale=1.0):
    """n values exactly representable in float32, every gap > 1e-7 * 10"""
    x = _f32(rng.permutation(n) * (scale / n) + rng.uniform(0.1, 0.4, n) * (scale / n))
    assert np.diff(np.sort(x)).min() > 1e-6 * scale
    return x


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - b) ** 2)))


def test_exact_parity_one_input():
    from sklearn.tree import DecisionTreeRegressor
    rng = np.random.default_rng(1)
    M = 257
    x = _distinct_f32(rng, M + N_TEST)
    y = np.sin(7 * x) + 0.1 * rng.standard_normal(M + N_TEST)
    tree = tt.fit_tree(x[:M], y[:M])
    sk = DecisionTreeRegressor().fit(x[:M, None], y[:M]).predict(x[M:, None])
    assert np.abs(tt.predict_tree(tree, x[M:])[:, 0] - sk).max() <= 1e-12
    assert tt.check_tree(tree, x[:M], y[:M])["leaves"] == M


def test_exact_parity_two_inputs_one_rounded():
    from sklearn.tree import DecisionTreeRegressor
    rng = np.random.default_rng(2)
    M = 300
    X = np.column_stack((_distinct_f32(rng, M + N_TEST), _f32(np.round(rng.uniform(0, 1, M + N_TEST) * 40) / 40)))
    # (two rows that differ in BOTH inputs tie exactly across them, and scikit-learn draws such ties at random: the levels of the
    # rounded input are 2.5 apart in the target, more than the rest of it spans, so the tree separates the levels first and
    # every small node lies inside one level, where only the other input has candidates -- the tree is unique)
    Y = (100 * X[:, 1] + np.sin(5 * X[:, 0]) + 0.1 * rng.standard_normal(M + N_TEST))[:, None]
    tree = tt.fit_tree(X[:M], Y[:M])
    mine = tt.predict_tree(tree, X[M:])[:, 0]
    differing = [int((np.abs(DecisionTreeRegressor(random_state=s).fit(X[:M], Y[:M, 0]).predict(X[M:]) - mine) > 1e-12).sum())
                 for s in range(5)]
    print("differing held-out rows of 100 per random_state:", differing)
    assert max(differing) == 0
    tt.check_tree(tree, X[:M], Y[:M])


def _band_data(M, m, q, seed):
    """Unit-scale inputs in (-0.7, 1.3) (the range of the synthetic blocks of test_gpu_poly_map.py), all gaps > 1e-6."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([_f32(2 * _distinct_f32(rng, M + 1000) - 0.7) for _ in range(m)])
    k = np.arange(q)
    Y = np.sin(3 * (k + 1) * X[:, :1]) + k * X[:, m - 1:m] ** 2 + 0.1 * rng.standard_normal((M + 1000, q))
    return X, Y


@pytest.mark.parametrize("M,m,q", [(1025, 4, 20), (600, 3, 4)], ids=["m1025", "m600"])
def test_band_against_scikit_learn(M, m, q):
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    X, Y = _band_data(M, m, q, seed=M)
    Xtr, Ytr, Xte, Yte = X[:M], Y[:M], X[M:], Y[M:]
    truth = _rmse(tt.predict_tree(tt.fit_tree(Xtr, Ytr), Xte), Yte)
    sk = [_rmse(DecisionTreeRegressor(random_state=s).fit(Xtr, Ytr).predict(Xte).reshape(Yte.shape), Yte) for s in range(20)]
    print(f"tree M = {M}: truth {truth:.4f}, scikit-learn {min(sk):.4f} .. {max(sk):.4f}")
    assert abs(truth / np.median(sk) - 1) <= 0.10
    from romhighcontrast_amd.nonlinear import ForestMap
    forest = tt.fit_forest(Xtr, Ytr, ForestMap.bootstrap_counts(10, M, 0))
    truth_f = _rmse(tt.predict_forest(forest, Xte), Yte)
    sk_f = [_rmse(RandomForestRegressor(n_estimators=10, random_state=s).fit(Xtr, Ytr).predict(Xte).reshape(Yte.shape), Yte)
            for s in range(20)]
    print(f"forest M = {M}: truth {truth_f:.4f}, scikit-learn {min(sk_f):.4f} .. {max(sk_f):.4f}")
    assert abs(truth_f / np.median(sk_f) - 1) <= 0.10


def test_checker_accepts_the_truth_and_rejects_mutations():
    rng = np.random.default_rng(3)
    M, m, q = 200, 3, 2
    X = rng.uniform(-1, 1, (M, m))
    Y = np.column_stack((np.sin(4 * X[:, 0]) + X[:, 1], X[:, 2] ** 2)) + 0.05 * rng.standard_normal((M, q))
    counts = np.bincount(rng.integers(0, M, M), minlength=M)
    for cnt, kw in ((None, {}), (counts, {}), (None, dict(max_depth=3)), (counts, dict(min_samples_leaf=7, min_samples_split=20))):
        tree = tt.fit_tree(X, Y, cnt, **kw)
        stats = tt.check_tree(tree, X, Y, cnt, **kw)
        assert stats["worst_gain"] == 0.0, stats
    tree = tt.fit_tree(X, Y)

    def mutated(**changes):
        t = {k: v.copy() for k, v in tree.items()}
        for k, (i, v) in changes.items():
            t[k][i] = v
        return t

    # one threshold moved across a row: the smallest value of its input above the root's threshold, in the root's rows
    f0 = tree["feature"][0]
    above = np.sort(X[X[:, f0] > tree["threshold"][0], f0])
    with pytest.raises(AssertionError):
        tt.check_tree(mutated(threshold=(0, above[0] + (above[1] - above[0]) / 2)), X, Y)
    # one leaf value off by 1e-9 relative
    leaf = int(np.flatnonzero(tree["feature"] < 0)[5])
    v = tree["value"][leaf].copy()
    v[0] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="leaf"):
        tt.check_tree(mutated(value=(leaf, v)), X, Y)
    # the root takes its second-best candidate (the rest greedy below it)
    second, gap = tt.fit_tree(X, Y, root_rank=1)
    assert gap > 1e-6, gap
    with pytest.raises(AssertionError, match="gain short"):
        tt.check_tree(second, X, Y)
    # a wrong count
    with pytest.raises(AssertionError, match="count"):
        tt.check_tree(mutated(count=(1, tree["count"][1] + 1)), X, Y)


def test_bootstrap_draw():
    from romhighcontrast_amd.nonlinear import ForestMap, TreeMap
    a, b = ForestMap.bootstrap_counts(10, 333, 0), ForestMap(10)._counts(333)
    assert a.dtype == np.int32 and a.shape == (10, 333) and np.array_equal(a, b) and (a.sum(1) == 333).all() and (a >= 0).all()
    assert not np.array_equal(a, ForestMap.bootstrap_counts(10, 333, 1)) and not np.array_equal(a[0], a[1])
    draw = np.random.default_rng(0).integers(0, 333, (10, 333))
    assert np.array_equal(a[3], np.bincount(draw[3], minlength=333))
    assert ForestMap(10, bootstrap=False)._counts(333) is None and TreeMap()._counts(333) is None
    assert TreeMap().steps[0][0] == "Tree device" and ForestMap().steps[0][0] == "RF device"
