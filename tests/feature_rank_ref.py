"""aleppo_feature_rank, restated: the float64 reference built from exported fc features, and the bounds a device answer has
to meet.  A plain helper module (no fixtures), shared by the CPU and GPU tests of tests/test_feature_rank.py.

With u = 2^-53 and n the rows that enter:
  Gram elements  |G - G_ref|_ij <= 2 n u (|Phi|^T |Phi|)_ij: both sides add n exact products (fp32 x fp32 is exact in
                 double) in some order, each within n u sum |terms| of the exact sum.
  column sums    |s - s_ref|_i <= 2 n u sum_r |Phi[r][i]|, by the same argument.
  eigenvalues    a backward-stable symmetric solver returns the exact eigenvalues of G + E, ||E||_2 <= p(H) u ||G||_2, so by
                 Weyl every eigenvalue moves by at most that; with the generous p(H) = 8 H per side,
                   solver bound   b = 16 H u lambda_max            (library against numpy.linalg.eigvalsh on the SAME matrix)
                   route bound    b + ||E_G||_F                    (library against an SVD of the features)
                 where E_G is the Gram error above, ||E_G||_F <= 2 n u || |Phi|^T |Phi| ||_F, and Weyl again (||.||_2 <= ||.||_F).
                 Centred, Gc = G - s s^T / n adds the error of the subtracted term: with a_i = sum_r |Phi[r][i]|,
                 |s_i s_j / n - exact| <= (2 n + 4) u a_i a_j / n (two sums of n terms, a product, a quotient, and the
                 subtraction's own rounding, first order), so ||E_G||_F grows by (2 n + 4) u ||a||^2 / n.
  singular values  sigma = sqrt(max(lambda, 0)): |sqrt x - sqrt y| = |x - y| / (sqrt x + sqrt y) <= min(sqrt b, b / sigma_ref)
                 =: ds_i.  Below sqrt b a singular value is rounding noise: the accuracy limit of the Gram route.
Real-valued stats, by propagation of ds (B = the eigenvalue bound used):
  SIGMA_MAX, SIGMA_MIN   ds_1, ds_H
  MEAN_SQ_NORM           (sum_i bound(G_ii) + H u trace) / n     (the Gram bound on the diagonal, and the order of the H additions)
  STABLE_RANK            (H + stable) B / sigma_1^2 * (1 + 1e-9)   (|dS2| <= H B, |d sigma_1^2| <= B; first order)
  EFFECTIVE_RANK         erank * dHent * 1.01, dHent = sum_i max |g(x) - g(p_i)| over x in [p_i - dp_i, p_i + dp_i] clipped to
                         [0, 1], g(p) = -p ln p (concave: the maximum is at an end, or at 1/e where the interval holds it),
                         dp_i = ds_i / S1 + p_i dS1 / S1, dS1 = sum ds_i; then |d exp(Hent)| <= erank * dHent to first order
Integer ranks must be equal; margins(ref) first shows ON THE REFERENCE ALONE that every deciding quantity is further from its
threshold than its propagated bound (so a tie can neither hide nor cause a failure):
  SRANK      |cum1_k - (1 - delta) S1| > 2 dS1 for every k          PCA_RANK   |cum2_k - (1 - delta) S2| > 2 H B
  THRESHOLD  |sigma_i / sqrt n - eps| > ds_i / sqrt n               NUMERICAL  |sigma_i - tol| > ds_i + tol ds_1 / sigma_1
"""
import numpy as np

U = 2.0 ** -53
STATS = ("rows", "nonfinite_rows", "sigma_max", "sigma_min", "mean_sq_norm", "effective_rank", "srank", "pca_rank",
         "threshold_rank", "stable_rank", "numerical_rank")
IDX = {n: i for i, n in enumerate(STATS)}
INTEGER = ("rows", "nonfinite_rows", "srank", "pca_rank", "threshold_rank", "numerical_rank")
REAL = ("sigma_max", "sigma_min", "mean_sq_norm", "effective_rank", "stable_rank")


def finite_rows(phi):
    phi = np.asarray(phi, np.float32)
    return np.isfinite(phi).all(axis=1)


def gram(phi):
    """fc features float32 [rows, H] -> dict: G and s in float64 over the finite rows, their element bounds, n, nonfinite"""
    phi = np.asarray(phi, np.float32)
    ok = finite_rows(phi)
    P = phi[ok].astype(np.float64)
    A = np.abs(P)
    n = int(ok.sum())
    absG = A.T @ A
    a = A.sum(axis=0)
    return dict(G=P.T @ P, s=P.sum(axis=0), n=n, nonfinite=int((~ok).sum()), H=phi.shape[1],
                G_bound=2 * n * U * absG, s_bound=2 * n * U * a, absG_F=float(np.linalg.norm(absG)), a_sq=float(a @ a), P=P)


def center(G, s, n):
    """Gc[i][j] = G[i][j] - (s[i] * s[j]) / n"""
    return G - np.outer(s, s) / n


def gram_error_F(g, centered):
    """||E_G||_F of the module docstring for the matrix the spectrum is taken of"""
    n = g["n"]
    e = 2 * n * U * g["absG_F"]
    if centered and n:
        e += (2 * n + 4) * U * g["a_sq"] / n
    return e


def solver_bound(H, lam_max):
    return 16 * H * U * max(lam_max, 0.0)


def metrics(lam, H, n, nonfinite, trace, delta, eps):
    """eigenvalues (descending) -> (stats float64 [11], sigma [H]); the definitions of aleppo_feature_rank_stat"""
    stats = np.zeros(len(STATS))
    stats[IDX["rows"]], stats[IDX["nonfinite_rows"]] = n, nonfinite
    sigma = np.sqrt(np.maximum(np.asarray(lam, np.float64), 0.0))
    S1, S2 = sigma.sum(), (sigma * sigma).sum()
    if n == 0 or S1 == 0:
        return stats, np.zeros(H)
    p = sigma / S1
    nz = p > 0
    tol = max(n, H) * 2.0 ** -23 * sigma[0]
    c1, c2 = np.cumsum(sigma), np.cumsum(sigma * sigma)
    first = lambda hit: int(np.argmax(hit)) + 1 if hit.any() else H
    vals = dict(sigma_max=sigma[0], sigma_min=sigma[-1], mean_sq_norm=trace / n,
                effective_rank=np.exp(-(p[nz] * np.log(p[nz])).sum()), srank=first(c1 >= (1 - delta) * S1),
                pca_rank=first(c2 >= (1 - delta) * S2), threshold_rank=int((sigma / np.sqrt(n) > eps).sum()),
                stable_rank=S2 / sigma[0] ** 2, numerical_rank=int((sigma > tol).sum()))
    for k, v in vals.items():
        stats[IDX[k]] = v
    return stats, sigma


def _sigma_bound(sigma, B):
    with np.errstate(divide="ignore"):
        return np.minimum(np.sqrt(B), np.where(sigma > 0, B / np.where(sigma > 0, sigma, 1.0), np.inf))


def _g(p):
    p = np.clip(p, 0.0, 1.0)
    return np.where(p > 0, -p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def reference(phi=None, delta=0.01, eps=0.01, centered=False, gram_of=None, extra_F=0.0, float32_delta=True):
    """the reference of one call.  phi: the features (the Gram is formed here, and the route bound applies: B = solver
    bound + ||E_G||_F).  gram_of = (G, s, n, nonfinite): the spectrum of a GIVEN Gram (the solver bound alone).  delta and
    eps are rounded to float32 first, as the C struct holds them."""
    if float32_delta:
        delta, eps = float(np.float32(delta)), float(np.float32(eps))
    if gram_of is None:
        g = gram(phi)
        G, s, n, nonfinite, H = g["G"], g["s"], g["n"], g["nonfinite"], g["H"]
        err_F = gram_error_F(g, centered)
        diag_bound = float(np.diag(g["G_bound"]).sum())
    else:
        G, s, n, nonfinite = gram_of
        G, s, H, g, err_F, diag_bound = np.asarray(G, np.float64), np.asarray(s, np.float64), len(s), None, 0.0, 0.0
    M = center(G, s, n) if (centered and n) else G
    lam = np.linalg.eigvalsh(M)[::-1] if n else np.zeros(H)
    if phi is not None and n and gram_of is None:  # the spectrum from an SVD of the features themselves
        P = g["P"] - g["P"].mean(axis=0) if centered else g["P"]
        sv = np.linalg.svd(P, compute_uv=False)
        lam_svd = np.zeros(H)
        lam_svd[:len(sv)] = sv * sv
        lam = lam_svd
    trace = float(np.diag(G).sum())
    stats, sigma = metrics(lam, H, n, nonfinite, trace, delta, eps)
    B = solver_bound(H, lam[0] if n else 0.0) + err_F + extra_F
    ds = _sigma_bound(sigma, B)
    S1, S2 = sigma.sum(), (sigma * sigma).sum()
    tol = np.zeros(len(STATS))
    if n and S1 > 0:
        dS1 = ds.sum()
        p = sigma / S1
        dp = ds / S1 + p * dS1 / S1
        lo, hi = np.clip(p - dp, 0, 1), np.clip(p + dp, 0, 1)
        dev = np.maximum(np.abs(_g(lo) - _g(p)), np.abs(_g(hi) - _g(p)))
        inside = (lo < np.exp(-1)) & (hi > np.exp(-1))
        dev = np.where(inside, np.maximum(dev, np.exp(-1) - _g(p)), dev)
        tol[IDX["sigma_max"]], tol[IDX["sigma_min"]] = ds[0], ds[-1]
        tol[IDX["mean_sq_norm"]] = (diag_bound + H * U * abs(trace)) / n
        tol[IDX["stable_rank"]] = (H + stats[IDX["stable_rank"]]) * B / sigma[0] ** 2 * (1 + 1e-9)
        tol[IDX["effective_rank"]] = stats[IDX["effective_rank"]] * dev.sum() * 1.01
    return dict(stats=stats, sigma=sigma, lam=lam, B=B, ds=ds, tol=tol, n=n, H=H, delta=delta, eps=eps, gram=g,
                centered=centered, G=G, s=s)


def margins(ref):
    """the ties the integer ranks could hide, on the reference alone: a list of strings (empty: every margin holds)"""
    sigma, ds, B, n, H = ref["sigma"], ref["ds"], ref["B"], ref["n"], ref["H"]
    S1, S2 = sigma.sum(), (sigma * sigma).sum()
    if n == 0 or S1 == 0:
        return []
    bad = []
    c1, c2 = np.cumsum(sigma), np.cumsum(sigma * sigma)
    m = np.abs(c1 - (1 - ref["delta"]) * S1).min()
    if not m > 2 * ds.sum():
        bad.append(f"srank: margin {m:.3g} <= {2 * ds.sum():.3g}")
    m = np.abs(c2 - (1 - ref["delta"]) * S2).min()
    if not m > 2 * H * B:
        bad.append(f"pca_rank: margin {m:.3g} <= {2 * H * B:.3g}")
    m = np.abs(sigma / np.sqrt(n) - ref["eps"]) - ds / np.sqrt(n)
    if not m.min() > 0:
        bad.append(f"threshold_rank: sigma[{m.argmin()}] within its bound of eps")
    t = max(n, H) * 2.0 ** -23 * sigma[0]
    m = np.abs(sigma - t) - (ds + t * ds[0] / sigma[0])
    if not m.min() > 0:
        bad.append(f"numerical_rank: sigma[{m.argmin()}] = {sigma[m.argmin()]:.3g} within its bound of {t:.3g}")
    return bad


def check_gram(got_G, got_s, g):
    """the device's G / s against gram(phi): failures as strings"""
    bad = []
    got_G, got_s = np.asarray(got_G, np.float64), np.asarray(got_s, np.float64)
    if not np.array_equal(got_G.view(np.uint64), np.ascontiguousarray(got_G.T).view(np.uint64)):
        bad.append("gram: G != G^T bit for bit")
    d = np.abs(got_G - g["G"])
    if not (d <= g["G_bound"]).all():
        i, j = np.unravel_index(np.argmax(d - g["G_bound"]), d.shape)
        bad.append(f"gram[{i}][{j}]: {got_G[i, j]!r} vs {g['G'][i, j]!r}, bound {g['G_bound'][i, j]:.3g}")
    d = np.abs(got_s - g["s"])
    if not (d <= g["s_bound"]).all():
        i = int(np.argmax(d - g["s_bound"]))
        bad.append(f"colsum[{i}]: {got_s[i]!r} vs {g['s'][i]!r}, bound {g['s_bound'][i]:.3g}")
    return bad


def worst_gram(got_G, got_s, g):
    """the largest |device - reference| / bound of G and of s (0 / 0 counts as 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        rG = np.nan_to_num(np.abs(np.asarray(got_G) - g["G"]) / g["G_bound"], nan=0.0)
        rs = np.nan_to_num(np.abs(np.asarray(got_s) - g["s"]) / g["s_bound"], nan=0.0)
    return float(rG.max()), float(rs.max())


def check_spectrum(stats, sigma, ref):
    """the library's stats / sigma against reference(...): failures as strings.  The eigenvalues are compared as
    sigma^2 against lam at the bound B (negative reference eigenvalues count as their clamp's input: |max(l, 0) - ...|)"""
    bad = []
    stats, sigma = np.asarray(stats, np.float64), np.asarray(sigma, np.float64)
    d = np.abs(sigma * sigma - np.maximum(ref["lam"], 0.0))
    # (a reference eigenvalue below zero is rounding noise of size <= B itself: the clamp can move it by B at the most)
    if not (d <= ref["B"] + 4 * U * max(ref["lam"][0], 0.0)).all():  # (+ the rounding of sqrt and of the square)
        i = int(np.argmax(d))
        bad.append(f"sigma[{i}]^2: {sigma[i] ** 2!r} vs {ref['lam'][i]!r}, bound {ref['B']:.3g}")
    if (np.diff(sigma) > 0).any():
        bad.append("sigma is not descending")
    for k in INTEGER:
        if stats[IDX[k]] != ref["stats"][IDX[k]]:
            bad.append(f"{k}: {stats[IDX[k]]} vs {ref['stats'][IDX[k]]}")
    for k in REAL:
        if not abs(stats[IDX[k]] - ref["stats"][IDX[k]]) <= ref["tol"][IDX[k]]:
            bad.append(f"{k}: {stats[IDX[k]]!r} vs {ref['stats'][IDX[k]]!r}, bound {ref['tol'][IDX[k]]:.3g}")
    return bad


def worst_spectrum(stats, sigma, ref):
    """{what: largest |library - reference| / bound}"""
    out = {}
    if ref["B"] > 0:
        out["lambda"] = float((np.abs(np.asarray(sigma) ** 2 - np.maximum(ref["lam"], 0.0)) / ref["B"]).max())
    for k in REAL:
        if ref["tol"][IDX[k]] > 0:
            out[k] = float(abs(stats[IDX[k]] - ref["stats"][IDX[k]]) / ref["tol"][IDX[k]])
    return out


def rank_deficient_params(params, H, A, copies=8, zeros=2):
    """fc rows H-1, H-2, ... (`copies` of them) become copies of rows 0, 1, ... (weights and bias), and the `zeros` rows
    before those become zero with zero bias: the features have rank <= H - copies - zeros, and the zeroed units give exactly
    zero rows and columns of G.  -> (params, zeroed unit indices)"""
    import adam_ref as ar
    offs = ar.param_offsets(H, A)
    p = np.array(params, np.float32, copy=True)
    w, b = int(offs[6]), int(offs[7])
    for k in range(copies):
        dst, src = H - 1 - k, k
        p[w + dst * 3136:w + (dst + 1) * 3136] = p[w + src * 3136:w + (src + 1) * 3136]
        p[b + dst] = p[b + src]
    dead = [H - 1 - copies - k for k in range(zeros)]
    for z in dead:
        p[w + z * 3136:w + (z + 1) * 3136] = 0
        p[b + z] = 0
    return p, dead


def overflow_params(params, H, A, unit=5):
    """the conv biases zero and fc weight row `unit` at 3e38: the all-zero observation gives zero conv activations, so its
    feature row is the fc bias (finite); any sample with a positive conv3 activation overflows unit `unit`"""
    import adam_ref as ar
    offs = ar.param_offsets(H, A)
    p = np.array(params, np.float32, copy=True)
    for k, c in ((1, 32), (3, 64), (5, 64)):
        p[int(offs[k]):int(offs[k]) + c] = 0
    p[int(offs[6]) + unit * 3136:int(offs[6]) + (unit + 1) * 3136] = np.float32(3e38)
    return p
