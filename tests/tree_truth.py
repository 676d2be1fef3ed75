"""Host truth for rom_tree_fit / rom_tree_predict (numpy long double, 80-bit on x86): a plain recursive greedy CART with the
semantics of include/romhc.h, and a CERTIFICATE CHECKER for a downloaded tree.

Near-ties make the tree itself non-unique under rounding (every two-row node ties exactly across all inputs), so a device
tree is not compared node by node with a truth tree.  Instead every node is verified:
  * the children partition the parent's rows by (input, threshold) and the weighted counts agree exactly;
  * internal node: the candidate is valid (between consecutive distinct values lo < hi, threshold = lo + (hi - lo) / 2 or lo,
    both sides >= min_samples_leaf, no stop condition holds) and its 80-bit gain >= the best 80-bit gain over all valid
    candidates - TOL, TOL = 64 n eps SS_node (SS_node: centred weighted sum of squares over all targets, eps = 2^-53).
    With targets shifted by the node's mean |S| <= sqrt(p SS) and dS <= n eps sqrt(p SS) on the smaller side p, so the error
    of the gain is <= 4 n eps SS; the factor 16 over that is the project's usual C = 64;
  * leaf: one of the four stop conditions holds, or the best 80-bit gain <= TOL;
  * leaf value: |value - 80-bit weighted mean| <= 64 n eps max|y - mean| + eps |mean|, bit for bit when the targets of the
    leaf's rows are constant (a one-row leaf).
A tree is a dict of arrays in the order of rom_tree_download: feature (-1 at a leaf), threshold, left (right = left + 1, -1 at
a leaf), count, value (nodes, q); node 0 is the root."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
C = 64


def _as2d(A):
    A = np.asarray(A, dtype=np.float64)
    return A.reshape(-1, 1) if A.ndim == 1 else A


def node_candidates(X, Y, w, idx, msl):
    """All candidates of the node with rows idx: (gains (n - 1, m) long double, -1 where invalid; order (n, m); SS; n; mean).
    gains[i, f]: the split after position i of the rows sorted (stably) by input f."""
    Xn, wn = X[idx], w[idx].astype(LD)
    n = wn.sum()
    Yn = Y[idx].astype(LD)
    mean = (wn[:, None] * Yn).sum(0) / n
    Yc = Yn - mean
    SS = (wn[:, None] * Yc * Yc).sum()
    if len(idx) == 1:
        return np.full((0, X.shape[1]), -1, dtype=LD), np.zeros((1, X.shape[1]), dtype=np.int64), SS, n, mean
    order = np.argsort(Xn, axis=0, kind="stable")
    xs = np.take_along_axis(Xn, order, 0)
    ws = wn[order]
    nL = np.cumsum(ws, 0)[:-1]
    nR = n - nL
    S = np.cumsum(ws[:, :, None] * Yc[order], 0)
    SL = S[:-1]
    SR = S[-1][None] - SL
    valid = (xs[:-1] < xs[1:]) & (nL >= msl) & (nR >= msl)
    g = (SL * SL).sum(2) / nL + (SR * SR).sum(2) / np.where(nR > 0, nR, 1)
    return np.where(valid, g, LD(-1)), order, SS, n, mean


def threshold(lo, hi):
    t = lo + (hi - lo) / 2
    return t if t < hi else lo


def fit_tree(X, Y, counts=None, max_depth=0, min_samples_split=2, min_samples_leaf=1, root_rank=0):
    """The greedy in long double, breadth first.  root_rank = 1: the ROOT takes its second-best candidate (for the
    checker's mutation test); returns (tree, relative gap between the best and the candidate taken at the root)."""
    X, Y = _as2d(X), _as2d(Y)
    M, q = Y.shape
    w = np.ones(M, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    feat, thr, left, cnt, val = [], [], [], [], []
    queue = [(np.flatnonzero(w > 0), 0)]
    root_gap = 0.0
    at = 0
    while at < len(queue):
        idx, depth = queue[at]
        g, order, SS, n, mean = node_candidates(X, Y, w, idx, min_samples_leaf)
        Yn = Y[idx]
        const = bool((Yn.min(0) == Yn.max(0)).all())
        value = Yn[0].copy() if const else mean.astype(np.float64)
        split = n >= min_samples_split and (max_depth == 0 or depth < max_depth) and not const and g.size and g.max() >= 0
        f = pos = -1
        if split:
            flat = g.T.ravel()          # input-major: the first maximum is the lowest input, then the lowest position
            k = int(np.argmax(flat))
            if at == 0 and root_rank:
                alt = flat.copy()
                alt[flat >= flat[k]] = -1
                k2 = int(np.argmax(alt))
                assert alt[k2] >= 0, "no second candidate at the root"
                root_gap = float((flat[k] - alt[k2]) / flat[k])
                k = k2
            f, pos = divmod(k, g.shape[0])
        feat.append(f)
        cnt.append(float(n))
        val.append(value)
        if split:
            rows = idx[order[:, f]]
            lo, hi = X[rows[pos], f], X[rows[pos + 1], f]
            thr.append(threshold(lo, hi))
            left.append(len(queue))
            queue.append((np.sort(rows[:pos + 1]), depth + 1))
            queue.append((np.sort(rows[pos + 1:]), depth + 1))
        else:
            thr.append(0.0)
            left.append(-1)
        at += 1
    tree = dict(feature=np.array(feat, dtype=np.int64), threshold=np.array(thr), left=np.array(left, dtype=np.int64),
                count=np.array(cnt), value=np.array(val).reshape(len(val), q))
    return (tree, root_gap) if root_rank else tree


def fit_forest(X, Y, counts, **kw):
    return [fit_tree(X, Y, c, **kw) for c in counts]


def split_forest(nodes, T):
    """The dict of TreeMapHandle.nodes() -> a list of T trees with tree-relative child numbers."""
    first = np.asarray(nodes["first"], dtype=np.int64)
    trees = []
    for t in range(T):
        a, b = first[t], first[t + 1]
        left = np.asarray(nodes["left"][a:b], dtype=np.int64)
        trees.append(dict(feature=np.asarray(nodes["feature"][a:b], dtype=np.int64), threshold=np.asarray(nodes["threshold"][a:b]),
                          left=np.where(left >= 0, left - a, -1), count=np.asarray(nodes["count"][a:b]),
                          value=np.asarray(nodes["value"][a:b])))
    return trees


def leaves_of(tree, X):
    """The leaf every row of X ends in: x <= threshold goes left."""
    X = _as2d(X)
    node = np.zeros(X.shape[0], dtype=np.int64)
    rows = np.arange(X.shape[0])
    while True:
        f = tree["feature"][node]
        inner = f >= 0
        if not inner.any():
            return node
        go_left = X[rows, np.where(inner, f, 0)] <= tree["threshold"][node]
        node = np.where(inner, tree["left"][node] + np.where(go_left, 0, 1), node)


def predict_tree(tree, X):
    return tree["value"][leaves_of(tree, X)]


def predict_forest(trees, X):
    """Mean over the trees, summed in tree order (fp64, as the device)."""
    s = predict_tree(trees[0], X).copy()
    for t in trees[1:]:
        s = s + predict_tree(t, X)
    return s / float(len(trees))


def check_tree(tree, X, Y, counts=None, max_depth=0, min_samples_split=2, min_samples_leaf=1):
    """The certificate (module docstring).  Raises AssertionError naming the node; returns a dict of statistics."""
    X, Y = _as2d(X), _as2d(Y)
    M, q = Y.shape
    w = np.ones(M, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    feat, thr, left, cnt, val = (tree[k] for k in ("feature", "threshold", "left", "count", "value"))
    N = len(feat)
    assert len(thr) == len(left) == len(cnt) == N and val.shape == (N, q), "array sizes"
    seen = np.zeros(N, dtype=bool)
    stack = [(0, np.flatnonzero(w > 0), 0)]
    worst_gain, worst_value, leaves, deepest = 0.0, 0.0, 0, 0
    while stack:
        nd, idx, depth = stack.pop()
        assert 0 <= nd < N and not seen[nd], f"node {nd}: reached twice or out of range"
        seen[nd] = True
        deepest = max(deepest, depth)
        assert len(idx) > 0, f"node {nd}: no rows"
        g, order, SS, n, mean = node_candidates(X, Y, w, idx, min_samples_leaf)
        assert cnt[nd] == float(n), f"node {nd}: count {cnt[nd]} != {float(n)}"
        tol = C * float(n) * EPS * SS
        best = g.max() if g.size else LD(-1)
        Yn = Y[idx]
        const = bool((Yn.min(0) == Yn.max(0)).all())
        stop = n < min_samples_split or (max_depth and depth == max_depth) or best < 0 or const
        if feat[nd] < 0:
            leaves += 1
            assert left[nd] < 0, f"leaf {nd}: has a child"
            if not stop:
                assert best <= tol, f"leaf {nd} ({len(idx)} rows): no stop condition holds and the best gain {float(best):.3e} > tol {float(tol):.3e}"
            if const:
                assert np.array_equal(val[nd].view(np.uint64), Yn[0].view(np.uint64)), f"leaf {nd}: constant targets, value not bit for bit"
            else:
                dev = np.abs(val[nd].astype(LD) - mean)
                bound = C * float(n) * EPS * np.abs(Yn.astype(LD) - mean).max(0) + EPS * np.abs(mean)
                assert (dev <= bound).all(), f"leaf {nd}: value off by {float((dev / bound).max()):.3e} of its bound"
                worst_value = max(worst_value, float((dev / np.where(bound > 0, bound, 1)).max()))
            continue
        f = int(feat[nd])
        assert not stop, f"node {nd}: split although a stop condition holds"
        assert 0 <= f < X.shape[1] and left[nd] + 1 < N, f"node {nd}: input or children out of range"
        rows = idx[order[:, f]]
        nl = int((X[rows, f] <= thr[nd]).sum())
        assert 0 < nl < len(rows), f"node {nd}: a side is empty"
        lo, hi = X[rows[nl - 1], f], X[rows[nl], f]
        assert lo < hi and thr[nd] == threshold(lo, hi), f"node {nd}: threshold {thr[nd]!r} is not that of ({lo!r}, {hi!r})"
        gain = g[nl - 1, f]
        assert gain >= 0, f"node {nd}: the candidate is not valid (min_samples_leaf or equal values)"
        assert gain >= best - tol, f"node {nd} ({len(idx)} rows): gain short of the best by {float((best - gain) / tol):.3e} tol"
        if tol > 0:
            worst_gain = max(worst_gain, float((best - gain) / tol))
        L = int(left[nd])
        stack.append((L, np.sort(rows[:nl]), depth + 1))
        stack.append((L + 1, np.sort(rows[nl:]), depth + 1))
    assert seen.all(), "nodes that no row reaches"
    assert N == 2 * leaves - 1, "nodes != 2 leaves - 1"
    return dict(nodes=N, leaves=leaves, deepest=deepest, worst_gain=worst_gain, worst_value=worst_value)


def check_forest(trees, X, Y, counts=None, **kw):
    return [check_tree(t, X, Y, None if counts is None else counts[i], **kw) for i, t in enumerate(trees)]
