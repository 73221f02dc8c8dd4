"""numpy restatement of the epipolar RANSAC that flags dynamic pair constraints
(FlowConstraintsCollection::setStaticFlagFromRansac, robust_cvd_amd/csrc/cvd_epipolar.h).

The reference declares the method but never implemented it, so this file is its definition.  Per directed pair p with its n
constraints (in the collection's map order):
  1. pixels x_a = loc[0:2] * w, x_b = loc[2:4] * w in f64 (w = width of the "down" raster; loc.y carries 1 / w);
  2. Hartley normalisation per side over all n points (centroid to the origin, mean distance sqrt(2)); a zero mean distance or
     n < 8 leaves the pair all static with best = (-1, -1);
  3. hypothesis k draws 8 distinct indices with splitmix64(seed << 44 | p << 24 | k << 8 | c) mod n, c = 0, 1, ... 255;
  4. 8 x 9 Gaussian elimination with full pivoting in normalised coordinates, free column = 1 (invalid: pivot < 1e-12 x the
     largest |entry|, or fewer than 8 distinct draws; count -1, F = 0);
  5. rank 2 (F <- F (I - v v^T), v the smallest right singular vector), F_pix = T_b^T F T_a;
  6. inlier <=> max(d_a, d_b) <= thresh, d_b = |r| / |(F x_a)_01|, d_a = |r| / |(F^T x_b)_01|, r = x_b^T F x_a (a zero
     denominator or a NaN is an outlier);
  7. winner = largest count, lowest k on ties;
  8. one refit over the winner's inliers (needs >= 8 of them): smallest eigenvector of the 9 x 9 normal matrix in normalised
     coordinates, rank 2, denormalised, rescored; adopted when it is finite and its count >= the winner's (a hypothesis
     whose F is not finite is invalid as well);
  9. the adopted F's inliers are the pair's static flags.
The GPU takes the closed-form 3 x 3 eigenvector for step 5 and Jacobi for step 8; this file uses the SVD / eigh (and states
the closed form in rank2_closed_form, which tests/test_epipolar_reference.py checks against the SVD).
"""
import numpy as np

MASK64 = (1 << 64) - 1
MAX_DRAWS = 256
PIVOT_RTOL = 1e-12


def splitmix64(x):
    z = (int(x) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def draw_sample(seed, p, k, n):
    """The 8 distinct constraint indices of hypothesis k of pair p (n constraints), or None when 256 draws do not give 8."""
    key0 = ((int(seed) << 44) | (int(p) << 24) | (int(k) << 8)) & MASK64
    out = []
    for c in range(MAX_DRAWS):
        i = splitmix64(key0 | c) % n
        if i not in out:
            out.append(i)
            if len(out) == 8:
                return out
    return None


def pixels(loc, w):
    loc = np.asarray(loc, dtype=np.float32).astype(np.float64)
    return loc[:, 0:2] * float(w), loc[:, 2:4] * float(w)


def normalisation(x):
    """Hartley: T (3 x 3) with T x = s (x - c), mean distance sqrt(2); None when the mean distance is 0."""
    c = x.mean(axis=0)
    md = np.sqrt(((x - c) ** 2).sum(axis=1)).mean()
    if not md > 0.0:
        return None
    s = np.sqrt(2.0) / md
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def apply(T, x):
    return np.stack([T[0, 0] * x[:, 0] + T[0, 2], T[1, 1] * x[:, 1] + T[1, 2]], axis=1)


def design_rows(xa, xb):
    """Rows of x_b^T F x_a = 0 for F row-major: [u x, u y, u, v x, v y, v, x, y, 1]."""
    x, y = xa[:, 0], xa[:, 1]
    u, v = xb[:, 0], xb[:, 1]
    one = np.ones_like(x)
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, one], axis=1)


def solve_minimal(A):
    """Null vector of an 8 x 9 system by Gaussian elimination with full pivoting (first maximum in row-major order of the
    remaining block), the column left over set to 1.  None when a pivot is below PIVOT_RTOL x the largest |entry|."""
    A = np.array(A, dtype=np.float64)
    perm = np.arange(9)
    amax = 0.0
    for r in range(8):
        sub = np.abs(A[r:, r:])
        pr, pc = divmod(int(np.argmax(sub)), 9 - r)
        pr += r
        pc += r
        piv = abs(A[pr, pc])
        if r == 0:
            amax = piv
        if not piv > 0.0 or piv < PIVOT_RTOL * amax:
            return None
        A[[r, pr]] = A[[pr, r]]
        A[:, [r, pc]] = A[:, [pc, r]]
        perm[[r, pc]] = perm[[pc, r]]
        inv = 1.0 / A[r, r]
        for i in range(r + 1, 8):
            f = A[i, r] * inv
            A[i, r + 1:] -= f * A[r, r + 1:]
            A[i, r] = 0.0
    x = np.zeros(9)
    x[8] = 1.0
    for r in range(7, -1, -1):
        x[r] = -(A[r, 8] + A[r, r + 1:8] @ x[r + 1:8]) / A[r, r]
    f = np.zeros(9)
    f[perm] = x
    return f.reshape(3, 3)


def rank2(F):
    U, S, Vt = np.linalg.svd(F)
    v = Vt[2]
    return F - np.outer(F @ v, v)


def rank2_closed_form(F):
    """What the GPU does: v = unit eigenvector of the smallest eigenvalue of G = F^T F, the eigenvalue by the trigonometric
    formula and v as the longest cross product of two rows of G - lambda I; F (I - v v^T)."""
    G = F.T @ F
    q = np.trace(G) / 3.0
    p1 = G[0, 1] ** 2 + G[0, 2] ** 2 + G[1, 2] ** 2
    p2 = (G[0, 0] - q) ** 2 + (G[1, 1] - q) ** 2 + (G[2, 2] - q) ** 2 + 2.0 * p1
    v = np.array([0.0, 0.0, 1.0])
    if p2 > 0.0:
        p = np.sqrt(p2 / 6.0)
        B = (G - q * np.eye(3)) / p
        r = np.clip(np.linalg.det(B) / 2.0, -1.0, 1.0)
        lam = q + 2.0 * p * np.cos(np.arccos(r) / 3.0 + 2.0 * np.pi / 3.0)
        M = G - lam * np.eye(3)
        cands = [np.cross(M[0], M[1]), np.cross(M[0], M[2]), np.cross(M[1], M[2])]
        norms = [c @ c for c in cands]
        best = int(np.argmax(norms))
        if norms[best] > 0.0:
            v = cands[best] / np.sqrt(norms[best])
    return F - np.outer(F @ v, v)


def distances(F, xa, xb):
    """(d_a, d_b) in pixels: the distance of x_a to the epipolar line F^T x_b and of x_b to F x_a (reference
    utils/epipolar_geometry.py:182-222); inf / NaN where a line is degenerate."""
    ha = np.concatenate([xa, np.ones((xa.shape[0], 1))], axis=1)
    hb = np.concatenate([xb, np.ones((xb.shape[0], 1))], axis=1)
    lb = ha @ F.T          # F x_a: lines in image b
    la = hb @ F            # F^T x_b: lines in image a
    r = np.abs((hb * lb).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        db = r / np.hypot(lb[:, 0], lb[:, 1])
        da = r / np.hypot(la[:, 0], la[:, 1])
    return da, db


def inliers(F, xa, xb, thresh):
    da, db = distances(F, xa, xb)
    with np.errstate(invalid="ignore"):
        return np.maximum(da, db) <= thresh   # NaN compares false; a zero denominator gives inf (or NaN)


def pair_ransac(xa, xb, thresh, iterations=1024, seed=0, p=0):
    """Steps 2-9 on one pair given f64 pixel coordinates.  Returns a dict: counts [K] (-1 = invalid hypothesis), F [K, 3, 3]
    (F_pix per hypothesis, 0 when invalid), best (k, count of the adopted F), F_best (the adopted F_pix), flags [n] uint8,
    refit (True when the refit was adopted), Ta / Tb (None for a degenerate pair)."""
    xa = np.asarray(xa, np.float64)
    xb = np.asarray(xb, np.float64)
    n = xa.shape[0]
    K = int(iterations)
    out = dict(counts=np.full(K, -1, np.int64), F=np.zeros((K, 3, 3)), best=(-1, -1), F_best=np.zeros((3, 3)),
               flags=np.ones(n, np.uint8), refit=False, Ta=None, Tb=None)
    if n < 8:
        return out
    Ta, Tb = normalisation(xa), normalisation(xb)
    if Ta is None or Tb is None:
        return out
    out["Ta"], out["Tb"] = Ta, Tb
    na, nb = apply(Ta, xa), apply(Tb, xb)
    for k in range(K):
        idx = draw_sample(seed, p, k, n)
        if idx is None:
            continue
        Fn = solve_minimal(design_rows(na[idx], nb[idx]))
        if Fn is None:
            continue
        Fp = Tb.T @ rank2(Fn) @ Ta
        if not np.isfinite(Fp).all():
            continue
        out["F"][k] = Fp
        out["counts"][k] = int(inliers(Fp, xa, xb, thresh).sum())
    kbest = int(np.argmax(out["counts"]))          # first maximum = lowest k on ties
    cbest = int(out["counts"][kbest])
    if cbest < 0:
        return out
    F = out["F"][kbest]
    inl = inliers(F, xa, xb, thresh)
    count = cbest
    if cbest >= 8:
        A = design_rows(na[inl], nb[inl])
        w, V = np.linalg.eigh(A.T @ A)
        Fr = Tb.T @ rank2(V[:, 0].reshape(3, 3)) @ Ta
        inl_r = inliers(Fr, xa, xb, thresh)
        if np.isfinite(Fr).all() and int(inl_r.sum()) >= cbest:   # a non-finite refit is never adopted
            F, inl, count = Fr, inl_r, int(inl_r.sum())
            out["refit"] = True
    out["best"] = (kbest, count)
    out["F_best"] = F
    out["flags"] = inl.astype(np.uint8)
    return out


def epipolar_static_flags(offsets, loc, pixel_scale, thresh, iterations=1024, seed=0, pairs=None):
    """Every pair (or the listed pair indices) of a collection: (flags [C] uint8, F [P, 3, 3], best [P, 2], per-pair dicts).
    Flags of pairs not listed stay 1."""
    offsets = np.asarray(offsets, np.int64)
    loc = np.asarray(loc, np.float32)
    if not np.isfinite(loc).all():
        raise ValueError("non-finite constraint location")
    P = offsets.shape[0] - 1
    flags = np.ones(loc.shape[0], np.uint8)
    F = np.zeros((P, 3, 3))
    best = np.full((P, 2), -1, np.int64)
    res = {}
    for p in (range(P) if pairs is None else pairs):
        a, b = int(offsets[p]), int(offsets[p + 1])
        xa, xb = pixels(loc[a:b], pixel_scale)
        r = pair_ransac(xa, xb, thresh, iterations, seed, p)
        flags[a:b] = r["flags"]
        F[p] = r["F_best"]
        best[p] = r["best"]
        res[p] = r
    return flags, F, best, res


def unit_sign(F):
    """F / |F| with the sign that makes the entry of largest magnitude positive (for comparisons up to scale)."""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    n = np.linalg.norm(F, axis=1, keepdims=True)
    G = np.divide(F, n, out=np.zeros_like(F), where=n > 0)
    s = np.sign(G[np.arange(G.shape[0]), np.abs(G).argmax(axis=1)])
    return G * np.where(s == 0, 1.0, s)[:, None]
