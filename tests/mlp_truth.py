"""Truth for rom_mlp_* (helper, not a test file): an 80-bit (np.longdouble) forward / backward pass of the MLP loss, written
independently of romhighcontrast_amd/nonlinear.py, the absolute-value propagation G_abs that scales the error bound, and the
fixed cases shared by tests/test_mlp_host.py (CPU) and tests/test_gpu_mlp.py.

THE BOUND, per gradient entry and for the loss:  |computed - truth| <= (M + sum_l K_l + 32) eps G_abs,  eps = 2^-53:
M eps for a sum over M rows in any order, sum K eps for the dot products along the depth, 32 eps for the activation and its
derivative at a few ulp each relative to their maxima.  G_abs is the same recursion as the truth with |x|, |W|, |b|, |y|, the
hidden activations replaced by min(z, 1) (tanh, logistic) or z (relu) and the derivative by its maximum 1, 1/4, 1.
The prediction: |computed - truth| <= (sum_l K_l + 32) eps (|y_mean| + y_scale * abs-propagated output) per entry."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
RELU_MARGIN = 2.0 ** -30


def split(w, sizes):
    """flat parameters -> [W_l (outputs, inputs)], [b_l]: all W in layer order, row-major, then all b"""
    Ws, bs, at = [], [], 0
    for k, n in zip(sizes[:-1], sizes[1:]):
        Ws.append(w[at:at + n * k].reshape(n, k))
        at += n * k
    for n in sizes[1:]:
        bs.append(w[at:at + n])
        at += n
    assert at == len(w)
    return Ws, bs


def count(sizes):
    """(P, offsets of W_l, offsets of b_l) by a plain Python count"""
    wo, at = [], 0
    for k, n in zip(sizes[:-1], sizes[1:]):
        wo.append(at)
        at += n * k
    bo = []
    for n in sizes[1:]:
        bo.append(at)
        at += n
    return at, wo, bo


def glorot(sizes, activation, seed, gain=1.0):
    """fixed random weights: uniform in +- gain sqrt(6 / (fan_in + fan_out)) (2 for logistic), flat"""
    rng = np.random.default_rng(seed)
    f = 2.0 if activation == "logistic" else 6.0
    Ws = [rng.uniform(-1, 1, (n, k)) * gain * np.sqrt(f / (n + k)) for k, n in zip(sizes[:-1], sizes[1:])]
    bs = [rng.uniform(-1, 1, n) * gain * np.sqrt(f / (n + k)) for k, n in zip(sizes[:-1], sizes[1:])]
    return np.concatenate([W.ravel() for W in Ws] + bs)


def scalings(X, Y, scale_targets=True):
    """c, h, y_mean, y_scale of the training rows in fp64 (c and h bit for bit what the device forms)"""
    mn, mx = X.min(axis=0), X.max(axis=0)
    c, h = 0.5 * mn + 0.5 * mx, 0.5 * mx - 0.5 * mn
    if not scale_targets:
        return c, h, np.zeros(Y.shape[1]), np.ones(Y.shape[1])
    const = Y.min(axis=0) == Y.max(axis=0)
    mean = np.where(const, Y[0], Y.mean(axis=0))
    sd = np.sqrt(((Y - mean) ** 2).mean(axis=0))
    return c, h, mean, np.where(const, 1.0, sd)


def scale_inputs(X, c, h):
    """t = (x - c) / h in fp64 (each operation correctly rounded: the device's bits), 0 for a constant column"""
    return np.where(h > 0.0, (X - c) / np.where(h > 0.0, h, 1.0), 0.0)


def scale_targets(Y, mean, scale):
    return (Y - mean) / scale


def _act(z, activation):
    if activation == "tanh":
        return np.tanh(z)
    if activation == "logistic":
        return 1 / (1 + np.exp(-z))
    return np.maximum(z, 0)


def forward(w, sizes, activation, T, dtype=LD, check_relu=True):
    """network outputs (M, q) and the hidden activations, in `dtype`.  relu in long double: asserts that every hidden
    pre-activation is at least 2^-30 from the kink (otherwise fp64 and the truth may take different branches)."""
    Ws, bs = split(np.asarray(w, dtype=dtype), sizes)
    A = [np.asarray(T, dtype=dtype)]
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = A[-1] @ W.T + b      # (NumPy's own loops: there is no BLAS in long double)
        if l + 1 < len(Ws):
            if activation == "relu" and check_relu and np.dtype(dtype) == np.dtype(LD):
                assert np.abs(z).min() > RELU_MARGIN, f"a relu pre-activation within 2^-30 of 0 ({np.abs(z).min():.3e}): another seed"
            z = _act(z, activation)
        A.append(z)
    return A[-1], A[:-1]


def loss_grad(w, sizes, activation, T, Ys, alpha, dtype=LD):
    """(L, gradient) of L = 1/(2M) sum |net(T) - Ys|^2 + alpha/(2M) sum |W_l|^2 in `dtype`"""
    w = np.asarray(w, dtype=dtype)
    Ws, _ = split(w, sizes)
    out, A = forward(w, sizes, activation, T, dtype)
    M = dtype(len(T))
    delta = out - np.asarray(Ys, dtype=dtype)
    pen = sum((W ** 2).sum() for W in Ws)
    L = ((delta ** 2).sum() / 2 + dtype(alpha) * pen / 2) / M
    gW, gb = [], []
    for l in range(len(Ws) - 1, -1, -1):
        gW.insert(0, ((delta.T @ A[l] + dtype(alpha) * Ws[l]) / M).ravel())
        gb.insert(0, delta.sum(axis=0) / M)
        if l > 0:
            a = A[l]
            der = 1 - a * a if activation == "tanh" else a * (1 - a) if activation == "logistic" else (a > 0).astype(dtype)
            delta = (delta @ Ws[l]) * der
    return L, np.concatenate(gW + gb)


def abs_propagation(w, sizes, activation, T, Ys, alpha):
    """(L_abs, G_abs (P,), abs-propagated outputs (M, q)) in long double"""
    w = np.abs(np.asarray(w, dtype=LD))
    Ws, bs = split(w, sizes)
    A = [np.abs(np.asarray(T, dtype=LD))]
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z = A[-1] @ W.T + b
        if l + 1 < len(Ws) and activation != "relu":
            z = np.minimum(z, 1)
        A.append(z)
    out = A[-1]
    M = LD(len(T))
    delta = out + np.abs(np.asarray(Ys, dtype=LD))
    L = ((delta ** 2).sum() / 2 + LD(alpha) * sum((W ** 2).sum() for W in Ws) / 2) / M
    dmax = LD(0.25) if activation == "logistic" else LD(1)
    gW, gb = [], []
    for l in range(len(Ws) - 1, -1, -1):
        gW.insert(0, ((delta.T @ A[l] + LD(alpha) * Ws[l]) / M).ravel())
        gb.insert(0, delta.sum(axis=0) / M)
        if l > 0:
            delta = (delta @ Ws[l]) * dmax
    return L, np.concatenate(gW + gb), out


def bound_factor(sizes, M):
    return (M + sum(sizes[:-1]) + 32) * EPS


def ratios(loss, grad, w, sizes, activation, T, Ys, alpha):
    """(|loss - truth| / bound, max over the entries of |grad - truth| / bound) for a computed loss and gradient"""
    Lt, Gt = loss_grad(w, sizes, activation, T, Ys, alpha)
    La, Ga, _ = abs_propagation(w, sizes, activation, T, Ys, alpha)
    f = LD(bound_factor(sizes, len(T)))
    rl = float(abs(LD(loss) - Lt) / (f * La))
    rg = float((np.abs(np.asarray(grad, dtype=LD) - Gt) / (f * Ga)).max())
    return rl, rg


# ---- the fixed cases of the loss / gradient test ------------------------------------------------------------------------
#          id                 m   hidden         q    M     activation  gain alpha seed
CASES = [("relu_3_7_5",       3,  [7],           5,   33,   "relu",     1.0, 0.0,  1),
         ("tanh_4_20_20_77",  4,  [20, 20],      77,  4101, "tanh",     1.0, 1e-2, 2),
         ("logistic_16_64_64_16", 16, [64, 64],  16,  1025, "logistic", 6.0, 1e-4, 3),
         ("tanh_16_17_33_15_17", 16, [17, 33, 15], 17, 2049, "tanh",    1.0, 1e-4, 4),
         ("relu_1_64_128",    1,  [64],          128, 97,   "relu",     1.0, 1e-4, 5),
         ("tanh_64_16_1",     64, [16],          1,   31,   "tanh",     1.0, 1e-4, 6),
         ("tanh_2_3_2_m1",    2,  [3],           2,   1,    "tanh",     1.0, 1e-4, 7)]
CONSTANT_COLUMNS_CASE = "tanh_16_17_33_15_17"   # input column 2 and target column 3 are constant there
HELD_OUT = 77                                   # rows after the M training rows of every case


def case_data(case):
    """X (M + HELD_OUT, m), Y (M + HELD_OUT, q) of a smooth map + noise, and the fixed weights w"""
    cid, m, hidden, q, M, activation, gain, alpha, seed = case
    rng = np.random.default_rng(1000 + seed)
    rows = M + HELD_OUT
    X = rng.uniform(-1, 1, (rows, m)) * (1.0 + np.arange(m)) + 0.25 * np.arange(m)
    mix = rng.standard_normal((m, q)) / np.sqrt(m)
    Y = np.sin(X / (1.0 + np.arange(m)) @ mix) + 0.3 * (X / (1.0 + np.arange(m)) @ mix) ** 2 + 0.05 * rng.standard_normal((rows, q))
    Y = Y * (1.0 + 0.5 * np.arange(q)) + np.arange(q)
    if cid == CONSTANT_COLUMNS_CASE:
        X[:, 2] = 1.75
        Y[:, 3] = -0.5
    sizes = [m] + list(hidden) + [q]
    return X, Y, glorot(sizes, activation, seed, gain), sizes


# ---- the fixed cases of the optimiser test ------------------------------------------------------------------------------
#              id              m  hidden    q  M    activation  seed
OPT_CASES = [("opt_tanh_300",  4, [20, 20], 5, 300, "tanh",     0),
             ("opt_logistic_33", 3, [7],    2, 33,  "logistic", 0)]
OPT_ALPHA, OPT_TOL, OPT_MEMORY = 1e-4, 1e-6, 10


def smooth_map(X, q):
    """a fixed smooth map R^m -> R^q"""
    m = X.shape[1]
    cols = []
    for j in range(q):
        a, b = X[:, j % m], X[:, (j + 1) % m]
        cols.append(np.sin(2.0 * a) * b + np.cos(a + (j + 1) * 0.5 * b) + 0.3 * a * a * (j + 1))
    return np.stack(cols, axis=1)


def opt_data(case, rows=None):
    cid, m, hidden, q, M, activation, seed = case
    rng = np.random.default_rng(2000 + seed + M)
    X = rng.uniform(-1, 1, (M if rows is None else rows, m))
    return X, smooth_map(X, q), [m] + list(hidden) + [q]
