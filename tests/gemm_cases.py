"""Cases and exact references of the GEMM conformance tests (test_gemm_cases.py on the CPU, test_gpu_gemm_exact.py on
the device).  NumPy only.

Operands are integers in [-8, 8] stored as fp32, C0 integers in [-64, 64], alpha in {1, -1, 0.5}, beta in {0, 2}: every
product and every partial sum of a case is an integer (or a half) below 2^24, hence exact in fp32 in ANY order.  The
right answer then does not depend on tile, k split, slab order or summation order, and a kernel is compared with the
float64 product bit for bit at every forced configuration.

Layout: an operand row holds K values and NaN from K up to its leading dimension (roundup4(K), or that plus 4; an odd
one or a base shifted by one float where the unaligned kernels are meant); C lies in a buffer of M + 2 rows of ldc
floats (ldc = N or N + 3) filled with a sentinel, its M x N window NaN when beta == 0.

The shapes are the smallest at which each mechanism of a kernel exists; from their cross product a fixed-seed sample
is taken in which every pair of values of two different axes occurs (`pairwise`)."""
import itertools

import numpy as np

SENTINEL = -12345.0
VMAX, CMAX = 8, 64
ALPHAS = (1.0, -1.0, 0.5)
BETAS = (0.0, 2.0)

# the instantiations of each kernel (test_gemm_cases.py holds them against the headers' own lists)
P_TILES = ((4, 4), (4, 3), (4, 2), (2, 4), (2, 3), (2, 2), (3, 3), (3, 2))
G_TILES = ((2, 2), (4, 2), (2, 4), (4, 4))
G_FORMS = ((1, 1), (1, 0), (0, 1), (0, 0))          # (ak, bk)
BATCHED_TRANS = ((0, 0), (0, 1), (1, 0), (1, 1))    # (transA, transB)
BATCHED_KGROUPS = (1, 2, 4)
KERNEL_P, KERNEL_NT, KERNEL_NT_H = 1, 2, 3

# 1, 2, 3 (the prologue's third load clamped), 4 and more k-tiles of 32, even and odd counts, ragged last tiles
NT_K = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 96, 97, 127, 129, 200, 419)
NT_SPLITS = (1, 2, 3, 5)
G_K = (1, 4, 31, 32, 33, 64, 97, 200)


def roundup4(n):
    return (n + 3) // 4 * 4


def pairwise(axes, seed, tries=60, total=0):
    """A fixed-seed list of dicts over `axes` ({name: values}) in which every pair of values of two different axes
    occurs (greedy: of `tries` random candidates that hold one pair still missing, the one that covers most), at least
    `total` cases long."""
    names = sorted(axes)
    rng = np.random.RandomState(seed)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in axes[a] for vb in axes[b]}

    def pairs(c):
        return {(a, c[a], b, c[b]) for a, b in itertools.combinations(names, 2)}
    out = []
    while todo:
        best, gain = None, -1
        first = min(todo, key=repr)                  # every round settles at least this one
        for _ in range(tries):
            c = {n: axes[n][rng.randint(len(axes[n]))] for n in names}
            c[first[0]], c[first[2]] = first[1], first[3]
            g = len(pairs(c) & todo)
            if g > gain:
                best, gain = c, g
        todo -= pairs(best)
        out.append(best)
    while len(out) < total:                          # topped up with plain random cases
        out.append({n: axes[n][rng.randint(len(axes[n]))] for n in names})
    return out


def uncovered_pairs(cases, axes):
    """The pairs of values of two different axes that no case holds (test_gemm_cases.py requires none)."""
    names = sorted(axes)
    seen = set()
    for c in cases:
        for a, b in itertools.combinations(names, 2):
            seen.add((a, c[a], b, c[b]))
    return [(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in axes[a] for vb in axes[b]
            if (a, va, b, vb) not in seen]


# ---------------------------------------------------------------------------------------------------------------
# C = alpha A B^T + beta C: k_gemm_p (one tile), k_gemm_nt, k_gemm_nt_h
# ---------------------------------------------------------------------------------------------------------------
def nt_axes(wm, wn):
    BM, BN = 32 * wm, 32 * wn
    return {"M": (1, BM - 1, BM, BM + 1, 2 * BM + 17),
            # N % 4 == 0 (16-byte store tail) and != 0 (scalar tail), on one tile and on several
            "N": (1, BN - 1, BN, BN + 1, 2 * BN + 17, 2 * BN + 20),
            "K": NT_K, "ksplit": NT_SPLITS, "xcd": (1, 2), "alpha": ALPHAS, "beta": BETAS,
            "pada": (0, 4), "padb": (0, 4), "padc": (0, 3)}


_NT_CACHE = {}


def nt_cases(kernel, wm=2, wn=2):
    """The cases of one k_gemm_p tile (kernel = KERNEL_P) or of the 64 x 64 kernels (wm = wn = 2)."""
    key = (kernel, wm, wn)
    if key not in _NT_CACHE:
        cs = pairwise(nt_axes(wm, wn), seed=1000 * kernel + 10 * wm + wn, total=150)
        for i, c in enumerate(cs):
            c.update(kernel=kernel, wm=wm, wn=wn, seed=100000 * kernel + 1000 * (10 * wm + wn) + i)
        _NT_CACHE[key] = cs
    return _NT_CACHE[key]


def _ints(rng, shape, vmax):
    return rng.randint(-vmax, vmax + 1, size=shape).astype(np.float64)


def padded(x, ld, fill=np.nan):
    """x [..., rows, cols] -> float32 [..., rows, ld], `fill` from cols up to ld"""
    out = np.full(x.shape[:-1] + (ld,), fill, dtype=np.float32)
    out[..., :x.shape[-1]] = x
    return out


def nt_data(c, lda_odd=False):
    """Operands, the initial C buffer and the exact result of a case.  a, b, c0: float64 integers; A, B: fp32 with NaN
    padding; Cbuf: [(M + 2), ldc] sentinel with the window set; want: the same buffer after a correct call."""
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.RandomState(c["seed"])
    a, b = _ints(rng, (M, K), VMAX), _ints(rng, (N, K), VMAX)
    c0 = _ints(rng, (M, N), CMAX)
    lda, ldb, ldc = roundup4(K) + c["pada"], roundup4(K) + c["padb"], N + c["padc"]
    if lda_odd:
        lda, ldb = lda + 1, ldb + 3
    Cbuf = np.full((M + 2, ldc), SENTINEL, dtype=np.float32)
    Cbuf[:M, :N] = c0 if c["beta"] != 0.0 else np.nan
    ref = c["alpha"] * (a @ b.T) + (c["beta"] * c0 if c["beta"] != 0.0 else 0.0)
    want = np.full((M + 2, ldc), SENTINEL, dtype=np.float32)
    want[:M, :N] = ref
    return dict(a=a, b=b, c0=c0, A=padded(a, lda), B=padded(b, ldb), lda=lda, ldb=ldb, ldc=ldc, Cbuf=Cbuf, ref=ref,
                want=want)


def slab_products(a, b, kchunk, nz):
    """[nz][M][N]: the exact product over each chunk's own k range"""
    K = a.shape[1]
    return np.stack([a[:, z * kchunk:min(K, (z + 1) * kchunk)] @ b[:, z * kchunk:min(K, (z + 1) * kchunk)].T
                     for z in range(nz)])


def exactness_margin(K, alpha, beta):
    """K 64 |alpha| + |beta| 64: below 2^24 every value a kernel can form on the way is an exact fp32 number"""
    return K * VMAX * VMAX * abs(alpha) + abs(beta) * CMAX


# ---------------------------------------------------------------------------------------------------------------
# k_gemm_g: C[g] = epilogue(opA(A[g]) opB(B[g]))
# ---------------------------------------------------------------------------------------------------------------
def g_axes(wm, wn, ak, bk):
    BM, BN = 32 * wm, 32 * wn
    # an m- / n-contiguous operand is fetched in whole 16-byte pieces: multiples of 4 only (the kernel's header)
    Ms = (1, BM - 1, BM, BM + 1, 2 * BM + 17) if ak else (4, BM - 4, BM, BM + 4, 2 * BM + 20)
    Ns = (1, BN - 1, BN, BN + 1, 2 * BN + 17) if bk else (4, BN - 4, BN, BN + 4, 2 * BN + 20)
    ax = {"M": Ms, "N": Ns, "K": G_K, "bias": (0, 1), "relu": (0, 1), "mask": (0, 1), "padc": (0, 3), "pada": (0, 4),
          "padb": (0, 4)}
    if not bk:
        ax["colsum"] = (0, 1)
    return ax


_G_CACHE = {}


def g_cases(wm, wn, ak, bk):
    key = (wm, wn, ak, bk)
    if key not in _G_CACHE:
        cs = pairwise(g_axes(wm, wn, ak, bk), seed=7000 + 100 * wm + 10 * wn + 2 * ak + bk)
        for i, c in enumerate(cs):
            c.setdefault("colsum", 0)
            c.update(wm=wm, wn=wn, ak=ak, bk=bk, groups=3, seed=500000 + 10000 * (4 * wm + wn) + 1000 * (2 * ak + bk) + i)
        _G_CACHE[key] = cs
    return _G_CACHE[key]


def checkerboard(M, N):
    """entries > 0, 0 and < 0 on the diagonals of a board"""
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    return ((m + 2 * n) % 3 - 1).astype(np.float64) * 3.0


def g_data(c):
    """The operands as they lie in memory (fp32, NaN padding), the sentinel-filled outputs and what they must hold
    after a correct call."""
    G, M, N, K, ak, bk = c["groups"], c["M"], c["N"], c["K"], c["ak"], c["bk"]
    rng = np.random.RandomState(c["seed"])
    a, b = _ints(rng, (G, M, K), VMAX), _ints(rng, (G, K, N), VMAX)          # opA(A), opB(B)
    bias = _ints(rng, (G, N), CMAX)
    lda = roundup4(K if ak else M) + c["pada"]
    ldb = roundup4(K if bk else N) + c["padb"]
    A = padded(a if ak else a.transpose(0, 2, 1), lda)
    B = padded(b.transpose(0, 2, 1) if bk else b, ldb)
    ldc, ldm, ldcs = N + c["padc"], N + 1, N + 3
    v = a @ b
    if c["bias"]:
        v = v + bias[:, None, :]
    if c["relu"]:
        v = np.maximum(v, 0.0)
    mask = np.stack([checkerboard(M, N) * (1 if g % 2 == 0 else -1) for g in range(G)])
    if c["mask"]:
        v = np.where(mask > 0, v, 0.0)
    want = np.full((G, M + 2, ldc), SENTINEL, dtype=np.float32)
    want[:, :M, :N] = v
    want_cs = np.full((G, ldcs), SENTINEL, dtype=np.float32)
    if c["colsum"]:
        want_cs[:, :N] = b.sum(axis=1)
    return dict(a=a, b=b, A=A, B=B, lda=lda, ldb=ldb, ldc=ldc, ldm=ldm, ldcs=ldcs, bias=bias.astype(np.float32),
                mask=padded(mask, ldm, fill=SENTINEL), Cbuf=np.full((G, M + 2, ldc), SENTINEL, dtype=np.float32),
                want=want, csbuf=np.full((G, ldcs), SENTINEL, dtype=np.float32), want_cs=want_cs, ref=v)


# ---------------------------------------------------------------------------------------------------------------
# k_gemm_batched_gen through aomarl_gemm_batched: C[b] = act(opA(A[b]) opB(B[b]) + bias[b]) (+ C[b])
# ---------------------------------------------------------------------------------------------------------------
def batched_axes():
    return {"M": (1, 63, 64, 65, 145), "N": (1, 63, 64, 65, 145), "K": G_K, "trans": BATCHED_TRANS,
            # each operand's leading dimension a multiple of 4 (128-bit loads) or odd (element-wise), independently
            "aligned_a": (0, 1), "aligned_b": (0, 1),
            "accumulate": (0, 1), "bias": (0, 1), "relu": (0, 1), "padc": (0, 3)}


_B_CACHE = {}


def batched_cases(kgroups):
    if kgroups not in _B_CACHE:
        cs = pairwise(batched_axes(), seed=9000 + kgroups)
        for i, c in enumerate(cs):
            c.update(kgroups=kgroups, batch=3, seed=900000 + 1000 * kgroups + i)
        _B_CACHE[kgroups] = cs
    return _B_CACHE[kgroups]


def batched_data(c):
    G, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    ta, tb = c["trans"]
    rng = np.random.RandomState(c["seed"])
    a, b = _ints(rng, (G, M, K), VMAX), _ints(rng, (G, K, N), VMAX)
    bias, c0 = _ints(rng, (G, N), CMAX), _ints(rng, (G, M, N), CMAX)
    lda = roundup4(M if ta else K) + 4 + (0 if c["aligned_a"] else 1)
    ldb = roundup4(N if tb else K) + (0 if c["aligned_b"] else 1)
    A = padded(a.transpose(0, 2, 1) if ta else a, lda)
    B = padded(b if tb else b.transpose(0, 2, 1), ldb)
    ldc = N + c["padc"]
    v = a @ b
    if c["bias"]:
        v = v + bias[:, None, :]
    if c["accumulate"]:
        v = v + c0
    if c["relu"]:
        v = np.maximum(v, 0.0)
    Cbuf = np.full((G, M + 2, ldc), SENTINEL, dtype=np.float32)
    Cbuf[:, :M, :N] = c0 if c["accumulate"] else np.nan
    want = np.full((G, M + 2, ldc), SENTINEL, dtype=np.float32)
    want[:, :M, :N] = v
    return dict(a=a, b=b, A=A, B=B, lda=lda, ldb=ldb, ldc=ldc, bias=bias.astype(np.float32), Cbuf=Cbuf, want=want, ref=v)


# ---------------------------------------------------------------------------------------------------------------
# the instantiations a case list reaches
# ---------------------------------------------------------------------------------------------------------------
def instantiation_counts():
    """{instantiation: number of cases that launch it} for every kernel, tile, form and k-group the conformance tests
    are to cover; test_gemm_cases.py fails on a zero."""
    n = {}
    for wm, wn in P_TILES:
        n["k_gemm_p<%d,%d>" % (wm, wn)] = len(nt_cases(KERNEL_P, wm, wn))
        n["k_gemm_p<%d,%d> split" % (wm, wn)] = sum(1 for c in nt_cases(KERNEL_P, wm, wn)
                                                    if c["ksplit"] > 1 and c["K"] > 32)
    n["k_gemm_nt"] = len(nt_cases(KERNEL_NT))
    n["k_gemm_nt_h"] = len(nt_cases(KERNEL_NT_H))
    for wm, wn in G_TILES:
        for ak, bk in G_FORMS:
            cs = g_cases(wm, wn, ak, bk)
            n["k_gemm_g<%d,%d,%d,%d>" % (wm, wn, ak, bk)] = len(cs)
            n["k_gemm_g<%d,%d,%d,%d> mask" % (wm, wn, ak, bk)] = sum(c["mask"] for c in cs)
            if not bk:
                n["k_gemm_g<%d,%d,%d,%d> colsum" % (wm, wn, ak, bk)] = sum(c["colsum"] for c in cs)
    for G in BATCHED_KGROUPS:
        for ta, tb in BATCHED_TRANS:
            n["k_gemm_batched_gen<%d,%d,%d>" % (ta, tb, G)] = sum(1 for c in batched_cases(G) if c["trans"] == (ta, tb))
    return n


# ---------------------------------------------------------------------------------------------------------------
# rounding quality: heavy-tailed operands, the a-priori bound of any fp32 summation order
# ---------------------------------------------------------------------------------------------------------------
def heavy_tailed(shape, seed, scale=1.0):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape)) * scale).astype(np.float32)


def rounding_bound(K, abs_products, alpha=1.0, beta_c0=0.0):
    """|err| <= (K + 4) 2^-24 (|alpha| sum |a||b| + |beta C0|): K - 1 additions, the products' roundings, alpha, beta C"""
    return (K + 4) * 2.0 ** -24 * (abs(alpha) * abs_products + np.abs(beta_c0))
