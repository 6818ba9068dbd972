"""Exact-arithmetic conformance of the library's five GEMM kernels: every instantiation, tile and k split, forced
through aomarl_gemm_nt_probe / aomarl_gemm_g_probe (and the "gemm_kgroups" option), against the float64 product
BIT FOR BIT.  The operands are small integers (tests/gemm_cases.py): every partial sum is exact in fp32, so the right
answer does not depend on tile, chunk, slab order or summation order, and one stale 16-byte piece, one column stored
past N, one chunk boundary off by four or one slab summed twice changes a result that has no tolerance to hide in.
NaN lies behind every operand row and, when beta == 0, in C; a sentinel lies round C and behind the slabs.

A second, loose tier checks rounding quality on heavy-tailed operands against the a-priori bound of fp32 summation,
(K + 4) 2^-24 (|alpha| sum |a||b| + |beta C0|), and prints the largest observed ratio per kernel."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import gemm_cases as gc  # noqa: E402

WS_TAIL = 64           # sentinel floats behind the workspace the library is told about


def _la():
    from ao_marl_amd import libaomarl as la
    return la, la.load()


def _stream():
    la, _ = _la()
    return la.raw_stream(torch.device("cuda:0"))


def _dev(x, offset=False):
    """NumPy -> device; offset: the same values at a base address one float past a 16-byte boundary"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not offset:
        return t.cuda()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _explain(got, want, M, N):
    """which property of an output buffer [.., M + 2, ldc] does not hold"""
    g, w = got.cpu().numpy(), want.cpu().numpy()
    win_g, win_w = g[..., :M, :N], w[..., :M, :N]
    out = []
    if np.isnan(win_g).any():
        out.append("%d NaN in C" % int(np.isnan(win_g).sum()))
    ne = win_g != win_w
    if ne.any():
        i = tuple(int(v) for v in np.argwhere(ne)[0])
        out.append("%d of %d values differ, first at %s: %r != %r" % (int(ne.sum()), ne.size, i, float(win_g[i]),
                                                                      float(win_w[i])))
    if (g[..., :M, N:] != w[..., :M, N:]).any():
        out.append("columns past N written")
    if (g[..., M:, :] != w[..., M:, :]).any():
        out.append("rows past M written")
    return "; ".join(out) or "equal"


def _report(bad, limit=6):
    assert not bad, "%d failures, first %d:\n%s" % (len(bad), min(limit, len(bad)), "\n".join(bad[:limit]))


def _brief(c):
    return ", ".join("%s=%s" % (k, c[k]) for k in sorted(c) if k != "seed")


class NtCall:
    """one case's operands on the device; run() calls aomarl_gemm_nt_probe on fresh C and workspace buffers"""

    def __init__(self, c, d, unaligned=None):
        self.c, self.d = c, d
        self.A, self.B = _dev(d["A"], offset=unaligned == "offset"), _dev(d["B"], offset=unaligned == "offset")
        self.Cbuf, self.want = _dev(d["Cbuf"]), _dev(d["want"])

    def run(self, kernel=0, wm=0, wn=0, ksplit=0, xcd=0, pick_M=0, slabs_only=0, sa=0.0, sb=0.0, work=True, ws_slabs=0,
            epi=None):
        la, lib = _la()
        c, d = self.c, self.d
        M, N, K = c["M"], c["N"], c["K"]
        Cd = self.Cbuf.clone()
        nws = max(ksplit, ws_slabs, 1) * M * N if work else 0      # room for exactly the chunks asked for
        ws = torch.full((nws + WS_TAIL,), gc.SENTINEL, device="cuda")
        pr = la.GemmProbe(kernel=kernel, wm=wm, wn=wn, ksplit=ksplit, xcd=xcd, pick_M=pick_M, slabs_only=slabs_only,
                          scale_a=sa, scale_b=sb, **(epi or {}))
        rc = lib.aomarl_gemm_nt_probe(M, N, K, c["alpha"], self.A.data_ptr(), d["lda"], self.B.data_ptr(), d["ldb"],
                                      c["beta"], Cd.data_ptr(), d["ldc"], ws.data_ptr() if work else None, nws,
                                      C.byref(pr), _stream())
        la.check(rc)
        return Cd, ws, pr


def _chunks_as_asked(pr, K, asked, unit):
    """whole k-tiles per chunk, every chunk non-empty, no more chunks than asked for and none longer than needed"""
    per = -(-K // asked)
    return (pr.r_kchunk % 32 == 0 and pr.r_kchunk == -(-per // unit) * unit and 1 <= pr.r_nz <= asked and
            (pr.r_nz - 1) * pr.r_kchunk < K <= pr.r_nz * pr.r_kchunk)


def _check_nt_case(bad, call, forced, kernel_want, unit, tile=(2, 2)):
    """One case through one forced configuration: result, guards, NaN, report, workspace tail, the slabs one by one,
    then the slabs-only mode."""
    c, d = call.c, call.d
    M, N, K, asked = c["M"], c["N"], c["K"], c["ksplit"]
    tag = _brief(c)
    Cd, ws, pr = call.run(**forced)
    if (pr.r_kernel, pr.r_wm, pr.r_wn) != (kernel_want,) + tuple(tile) or not _chunks_as_asked(pr, K, asked, unit):
        bad.append("%s: launched kernel %d tile %d x %d nz %d kchunk %d" % (tag, pr.r_kernel, pr.r_wm, pr.r_wn, pr.r_nz,
                                                                           pr.r_kchunk))
        return
    nz = pr.r_nz
    if not torch.equal(Cd, call.want):
        bad.append("%s (nz %d): %s" % (tag, nz, _explain(Cd, call.want, M, N)))
    used = nz * M * N if nz > 1 else 0
    if not bool((ws[used:] == gc.SENTINEL).all()):
        bad.append("%s (nz %d): workspace written past its %d slabs" % (tag, nz, nz if nz > 1 else 0))
    if nz == 1:
        Cs, _, ps = call.run(slabs_only=1, **forced)
        if ps.r_slabs != 0 or not torch.equal(Cs, call.want):
            bad.append("%s: slabs-only on an unsplit product: r_slabs %d, %s" % (tag, ps.r_slabs,
                                                                                 _explain(Cs, call.want, M, N)))
        return
    slabs = torch.from_numpy(gc.slab_products(d["a"], d["b"], pr.r_kchunk, nz).astype(np.float32)).cuda()
    sc = float(forced.get("sa") or 1.0) * float(forced.get("sb") or 1.0)      # k_gemm_nt_h's slabs carry the scales
    if not torch.equal(ws[:used].view(nz, M, N), slabs * sc):
        z = [i for i in range(nz) if not torch.equal(ws[:used].view(nz, M, N)[i], slabs[i] * sc)]
        bad.append("%s (nz %d, kchunk %d): slabs %s are not the product over their own k range" % (tag, nz, pr.r_kchunk, z))
    Cs, ws2, ps = call.run(slabs_only=1, **forced)
    if not _same_bits(Cs, call.Cbuf):
        bad.append("%s: slabs-only wrote to C" % tag)
    if (ps.r_slabs, ps.r_nz, ps.r_kchunk) != (nz, nz, pr.r_kchunk) or ps.r_alpha != np.float32(c["alpha"] / sc):
        bad.append("%s: slabs-only reports %d slabs (nz %d) alpha %r" % (tag, ps.r_slabs, ps.r_nz, ps.r_alpha))
        return
    P = ws2[:used].view(nz, M, N)
    total = ps.r_alpha * P.sum(0, dtype=torch.float32)
    prod = torch.from_numpy((c["alpha"] * (d["a"] @ d["b"].T)).astype(np.float32)).cuda()
    if not torch.equal(P, slabs * sc) or not torch.equal(total, prod) or not bool((ws2[used:] == gc.SENTINEL).all()):
        bad.append("%s (nz %d): slabs-only: slabs, their sum x alpha_out or the workspace tail wrong" % (tag, nz))


# ------------------------------------------------------------------------------------------------ k_gemm_p
@pytest.mark.parametrize("wm,wn", gc.P_TILES)
def test_gemm_p_tile_exact(wm, wn):
    """One forced tile of k_gemm_p over its case list: M, N round one and two tiles, 1 .. 14 k-tiles with ragged ends,
    1 .. 5 chunks asked for, both block numberings."""
    bad, nsplit = [], 0
    for c in gc.nt_cases(gc.KERNEL_P, wm, wn):
        call = NtCall(c, gc.nt_data(c))
        n0 = len(bad)
        _check_nt_case(bad, call, dict(kernel=gc.KERNEL_P, wm=wm, wn=wn, ksplit=c["ksplit"], xcd=c["xcd"]), gc.KERNEL_P,
                       unit=32, tile=(wm, wn))
        nsplit += len(bad) == n0 and c["ksplit"] > 1 and c["K"] > 32
    _report(bad)
    assert nsplit >= 20            # the split path was exercised, not only reported


def test_probe_refuses_what_it_cannot_force():
    la, lib = _la()
    c = dict(M=70, N=66, K=419, alpha=1.0, beta=0.0, pada=0, padb=0, padc=0, seed=1, ksplit=1)
    call = NtCall(c, gc.nt_data(c))
    for kw, word in ((dict(kernel=1, wm=3, wn=4), "wm"), (dict(kernel=1, wm=2, wn=0), "wm"),
                     (dict(kernel=2, wm=2, wn=2), "wm"), (dict(kernel=1, ksplit=3, work=False), "ksplit"),
                     (dict(kernel=4), "kernel"), (dict(xcd=3), "xcd"), (dict(pick_M=71), "pick_M"),
                     (dict(kernel=3, sa=3.0), "scale_a"), (dict(slabs_only=1, work=False), "slabs_only")):
        with pytest.raises(la.AomarlError, match=word):
            call.run(**kw)
    # a split whose slabs do not fit: 5 chunks asked for, room for 2
    Cd = call.Cbuf.clone()
    ws = torch.full((2 * 70 * 66 + WS_TAIL,), gc.SENTINEL, device="cuda")
    for kernel in (1, 2, 3):
        pr = la.GemmProbe(kernel=kernel, ksplit=5)
        rc = lib.aomarl_gemm_nt_probe(70, 66, 419, 1.0, call.A.data_ptr(), call.d["lda"], call.B.data_ptr(),
                                      call.d["ldb"], 0.0, Cd.data_ptr(), call.d["ldc"], ws.data_ptr(), 2 * 70 * 66,
                                      C.byref(pr), _stream())
        assert rc != 0 and "work_floats" in lib.aomarl_last_error().decode()
    torch.cuda.synchronize()
    assert _same_bits(Cd, call.Cbuf) and bool((ws == gc.SENTINEL).all())          # refused means nothing ran
    # an empty sum is refused by every door of the product (it used to divide by zero in the k split)
    for rc in (lib.aomarl_gemm_nt(70, 66, 0, 1.0, call.A.data_ptr(), call.d["lda"], call.B.data_ptr(), call.d["ldb"], 0.0,
                                  Cd.data_ptr(), call.d["ldc"], _stream()),
               lib.aomarl_gemm_nt_split(70, 66, 0, 1.0, call.A.data_ptr(), call.d["lda"], call.B.data_ptr(),
                                        call.d["ldb"], 0.0, Cd.data_ptr(), call.d["ldc"], 1.0, 1.0, None, 0, _stream())):
        assert rc != 0 and "K must be at least 1" in lib.aomarl_last_error().decode()
    with pytest.raises(la.AomarlError, match="sizes"):
        NtCall(dict(c, K=0), gc.nt_data(c)).run()
    assert _same_bits(Cd, call.Cbuf)
    # the aligned kernels on operands that are not
    odd = NtCall(c, gc.nt_data(c, lda_odd=True))
    for kernel in (1, 3):
        with pytest.raises(la.AomarlError, match="kernel"):
            odd.run(kernel=kernel)


@pytest.mark.parametrize("work", [True, False])
def test_pick_M_gives_the_parts_bits(work):
    """launch_gemm_nt's pick_M: 4 x 64 rows at once with the tile and k split of a 64-row product are, bit for bit,
    the four 64-row products -- on operands whose sums DO round."""
    la, lib = _la()
    M, Mp, N, K = 256, 64, 130, 1200
    g = torch.Generator().manual_seed(11)
    A, B = torch.randn(M, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda()
    per_part = 16 * Mp * N if work else 0

    def call(rows, a, pick_M, floats):
        out = torch.full((rows, N), float("nan"), device="cuda")
        ws = torch.zeros(max(floats, 1), device="cuda")
        pr = la.GemmProbe(pick_M=pick_M)
        la.check(lib.aomarl_gemm_nt_probe(rows, N, K, -1.0, a.data_ptr(), K, B.data_ptr(), K, 0.0, out.data_ptr(), N,
                                          ws.data_ptr() if floats else None, floats, C.byref(pr), _stream()))
        return out, pr
    whole, pw = call(M, A, Mp, 4 * per_part)
    parts = [call(Mp, A[i * Mp:(i + 1) * Mp], 0, per_part) for i in range(M // Mp)]
    cfg = lambda p: (p.r_kernel, p.r_wm, p.r_wn, p.r_nz, p.r_kchunk)  # noqa: E731
    print("pick_M: whole %s, part %s" % (cfg(pw), cfg(parts[0][1])))
    assert all(cfg(p) == cfg(pw) for _, p in parts) and pw.r_kernel == gc.KERNEL_P
    assert (pw.r_nz > 1) == work               # with its workspace this shape is split (so the slabs' order matters)
    assert torch.equal(whole, torch.cat([o for o, _ in parts]))
    ref = -(A.double() @ B.double().T)
    assert float((whole.double() - ref).abs().max()) < 1e-3


def test_unforced_path_and_its_memo():
    """33 shapes with a workspace (small ones, and three of the loop's size, where the cost model leaves the 64 x 64
    tile), visited twice in one process (the per-shape memo of launch_gemm_nt holds 16):
    exact results, the same configuration on the revisit, and the one gemm_p_pick gives (the probe reports it)."""
    shapes = [(M, N, K) for M in (1, 33, 64, 130, 256, 300) for N in (5, 90) for K in (3, 419)] + \
             [(M, 257, 1200) for M in (1, 33, 64, 130, 256, 300)] + [(256, 648, 1960), (512, 1286, 648), (512, 648, 648)]
    assert len(set(shapes)) == len(shapes) >= 20
    seen, bad, data = {}, [], {}
    for visit in range(2):
        for i, (M, N, K) in enumerate(shapes):
            c = dict(M=M, N=N, K=K, alpha=-1.0, beta=0.0 if i % 2 else 2.0, pada=0, padb=4, padc=3 * (i % 2), seed=40 + i,
                     ksplit=0)
            if i not in data:
                data[i] = gc.nt_data(c)
            call = NtCall(c, data[i])
            Cd, ws, pr = call.run(ws_slabs=16)
            cfg = (pr.r_kernel, pr.r_wm, pr.r_wn, pr.r_nz, pr.r_kchunk)
            if not torch.equal(Cd, call.want):
                bad.append("visit %d %s %s: %s" % (visit, (M, N, K), cfg, _explain(Cd, call.want, M, N)))
            if cfg != (gc.KERNEL_P, pr.p_wm, pr.p_wn, pr.p_nz, pr.p_kchunk):
                bad.append("visit %d %s: launched %s, gemm_p_pick gives %s" % (visit, (M, N, K), cfg,
                                                                             (pr.p_wm, pr.p_wn, pr.p_nz, pr.p_kchunk)))
            if seen.setdefault((M, N, K), cfg) != cfg:
                bad.append("%s: %s on the revisit, %s before" % ((M, N, K), cfg, seen[(M, N, K)]))
            used = pr.r_nz * M * N if pr.r_nz > 1 else 0
            if not bool((ws[used:] == gc.SENTINEL).all()):
                bad.append("visit %d %s: workspace written past its slabs" % (visit, (M, N, K)))
    _report(bad)
    assert len({cfg[1:3] for cfg in seen.values()}) >= 2 and any(cfg[3] > 1 for cfg in seen.values())


@pytest.mark.parametrize("kernel", [gc.KERNEL_P, gc.KERNEL_NT])
def test_reduce_epilogue_exact(kernel):
    """k_gemm_reduce_epi behind a split product: the integrator step (mode 1, one gain or one per row) and the agents'
    action (mode 2, an amode_inv with -1 entries), with integer gains and actions; an unsplit product leaves the step
    to the caller (r_fused == 0, com untouched)."""
    bad, fused = [], 0
    wm, wn = (2, 3) if kernel == gc.KERNEL_P else (2, 2)
    rng = np.random.RandomState(77)
    for c in gc.nt_cases(kernel, wm, wn)[::3]:
        M, N = c["M"], c["N"]
        d = gc.nt_data(c)
        call = NtCall(c, d)
        ldcom, nact = N + 3, 5
        com0 = np.full((M + 2, ldcom), gc.SENTINEL, dtype=np.float32)
        com0[:M, :N] = rng.randint(-64, 65, size=(M, N))
        grow = rng.randint(-3, 4, size=M).astype(np.float32)
        action = rng.randint(-8, 9, size=(M, nact)).astype(np.float32)
        freedom = rng.randint(-8, 9, size=N).astype(np.float32)
        inv = np.array([n % 7 if n % 7 < nact else -1 for n in range(N)], dtype=np.int32)
        t_grow, t_act, t_free, t_inv = _dev(grow), _dev(action), _dev(freedom), _dev(inv)
        ref = d["ref"]
        acted = ref + np.where(inv >= 0, action[:, np.maximum(inv, 0)] * freedom[None, :], 0.0)
        forced = dict(kernel=kernel, ksplit=c["ksplit"], xcd=c["xcd"])
        if kernel == gc.KERNEL_P:
            forced.update(wm=wm, wn=wn)
        for name, epi, gain, cref in (
                ("gain", dict(epi_mode=1, epi_gain=3.0), 3.0, ref),
                ("gain_row", dict(epi_mode=1, epi_gain=7.0, epi_gain_row=t_grow.data_ptr()), grow[:, None], ref),
                ("action", dict(epi_mode=2, epi_action=t_act.data_ptr(), epi_nact=nact, epi_amode_inv=t_inv.data_ptr(),
                                epi_freedom=t_free.data_ptr()), None, acted)):
            com = _dev(com0)
            if epi["epi_mode"] == 1:
                epi.update(epi_com=com.data_ptr(), epi_ldcom=ldcom)
            Cd, _, pr = call.run(epi=epi, **forced)
            want_c, want_com = d["want"].copy(), com0.copy()
            if pr.r_nz > 1:
                want_c[:M, :N] = cref
                if gain is not None:
                    want_com[:M, :N] += (gain * ref).astype(np.float32)
            if pr.r_fused != (pr.r_nz > 1) or not torch.equal(Cd, _dev(want_c)) or not torch.equal(com, _dev(want_com)):
                bad.append("%s, %s (nz %d, fused %d): C %s; com %s" % (
                    _brief(c), name, pr.r_nz, pr.r_fused, _explain(Cd, _dev(want_c), M, N), _explain(com, _dev(want_com), M, N)))
            fused += pr.r_fused
    _report(bad)
    assert fused >= 30


# ------------------------------------------------------------------------------------------------ k_gemm_nt, k_gemm_nt_h
@pytest.mark.parametrize("how", ["forced", "odd_ld", "offset"])
def test_gemm_nt_exact(how):
    """The element-wise fallback: forced on aligned operands, and reached on its own by odd leading dimensions and by
    a base address one float off; the shapes of the 64 x 64 tile, with and without split."""
    bad = []
    for c in gc.nt_cases(gc.KERNEL_NT):
        call = NtCall(c, gc.nt_data(c, lda_odd=how == "odd_ld"), unaligned=how)
        _check_nt_case(bad, call, dict(kernel=gc.KERNEL_NT if how == "forced" else 0, ksplit=c["ksplit"], xcd=c["xcd"]),
                       gc.KERNEL_NT, unit=32)
    _report(bad)


@pytest.mark.parametrize("sa,sb", [(1.0, 1.0), (512.0, 1.0), (1.0, 512.0), (512.0, 512.0)])
def test_gemm_nt_h_exact(sa, sb):
    """The split-fp16 kernel: integers up to 8 x 2^9 are exact in the hi half (lo = 0), every product and sum exact in
    fp32; nothing saturates."""
    la, _ = _la()
    la.gemm_saturated(_stream())
    bad = []
    for c in gc.nt_cases(gc.KERNEL_NT_H):
        call = NtCall(c, gc.nt_data(c))
        _check_nt_case(bad, call, dict(kernel=gc.KERNEL_NT_H, ksplit=c["ksplit"], xcd=c["xcd"], sa=sa, sb=sb),
                       gc.KERNEL_NT_H, unit=96)
    _report(bad)
    assert la.gemm_saturated(_stream()) == 0


# ------------------------------------------------------------------------------------------------ k_gemm_g
def _run_g(c, d, wm, wn):
    la, lib = _la()
    G, M, N, K = c["groups"], c["M"], c["N"], c["K"]
    A, B, Cd = _dev(d["A"]), _dev(d["B"]), _dev(d["Cbuf"])
    bias, mask, cs = _dev(d["bias"]), _dev(d["mask"]), _dev(d["csbuf"])
    a = la.GemmGArgs(groups=G, ak=c["ak"], bk=c["bk"], M=M, N=N, K=K,
                     A=A.data_ptr(), lda=d["lda"], sA=A.shape[1] * d["lda"],
                     B=B.data_ptr(), ldb=d["ldb"], sB=B.shape[1] * d["ldb"],
                     C=Cd.data_ptr(), ldc=d["ldc"], sC=(M + 2) * d["ldc"],
                     bias=bias.data_ptr() if c["bias"] else None, sBias=N, relu=c["relu"],
                     mask=mask.data_ptr() if c["mask"] else None, ldm=d["ldm"], sM=M * d["ldm"],
                     colsum=cs.data_ptr() if c["colsum"] else None, sCs=d["ldcs"], force_wm=wm, force_wn=wn)
    la.check(lib.aomarl_gemm_g_probe(C.byref(a), _stream()))
    torch.cuda.synchronize()
    return Cd, cs, (A, B, bias, mask)


@pytest.mark.parametrize("ak,bk", gc.G_FORMS)
@pytest.mark.parametrize("wm,wn", gc.G_TILES)
def test_gemm_g_exact(wm, wn, ak, bk):
    """One tile and operand form of the learner's grouped kernel, 3 groups: bias, ReLU, the > 0 mask and the column
    sums (written once: a sentinel is replaced, not added to)."""
    bad = []
    for c in gc.g_cases(wm, wn, ak, bk):
        d = gc.g_data(c)
        Cd, cs, _keep = _run_g(c, d, wm, wn)
        want, want_cs = _dev(d["want"]), _dev(d["want_cs"])
        if not torch.equal(Cd, want):
            bad.append("%s: %s" % (_brief(c), _explain(Cd, want, c["M"], c["N"])))
        if not torch.equal(cs, want_cs):
            bad.append("%s: column sums: %d of %d floats differ" % (_brief(c), int((cs != want_cs).sum()), cs.numel()))
    _report(bad)


def test_gemm_g_probe_refuses_what_the_kernel_cannot_take():
    la, lib = _la()
    c = dict(groups=3, M=64, N=64, K=32, ak=1, bk=0, bias=0, relu=0, mask=0, colsum=1, pada=0, padb=0, padc=0, seed=3)
    d = gc.g_data(c)
    A, B, Cd, cs = _dev(d["A"]), _dev(d["B"]), _dev(d["Cbuf"]), _dev(d["csbuf"])
    A1 = _dev(d["A"], offset=True)

    def args(**kw):
        a = dict(groups=3, ak=1, bk=0, M=64, N=64, K=32, A=A.data_ptr(), lda=32, sA=64 * 32, B=B.data_ptr(), ldb=64,
                 sB=32 * 64, C=Cd.data_ptr(), ldc=64, sC=66 * 64, colsum=cs.data_ptr(), sCs=67)
        a.update(kw)
        return la.GemmGArgs(**a)
    for kw, word in ((dict(A=A1.data_ptr()), "aligned"), (dict(lda=33), "lda"), (dict(ldb=66), "ldb"),
                     (dict(sA=64 * 32 + 2), "sA"), (dict(sB=32 * 64 + 1), "sB"), (dict(bk=1, ldb=32), "colsum"),
                     (dict(force_wm=3), "force_wm"), (dict(force_wn=8), "force_wn"), (dict(ak=0, lda=32), "lda"),
                     (dict(K=0), "sizes")):
        a = args(**kw)
        assert lib.aomarl_gemm_g_probe(C.byref(a), _stream()) != 0, kw
        assert word in lib.aomarl_last_error().decode(), (kw, lib.aomarl_last_error())
    torch.cuda.synchronize()
    assert bool((Cd == gc.SENTINEL).all()) and bool((cs == gc.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ k_gemm_batched_gen
def _run_batched(c, d):
    la, lib = _la()
    G, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    ta, tb = c["trans"]
    A, B, Cd, bias = _dev(d["A"]), _dev(d["B"]), _dev(d["Cbuf"]), _dev(d["bias"])
    la.check(lib.aomarl_gemm_batched(G, ta, tb, M, N, K, A.data_ptr(), d["lda"], A.shape[1] * d["lda"], B.data_ptr(),
                                     d["ldb"], B.shape[1] * d["ldb"], bias.data_ptr() if c["bias"] else None, N,
                                     Cd.data_ptr(), d["ldc"], (M + 2) * d["ldc"], c["relu"], c["accumulate"], _stream()))
    torch.cuda.synchronize()
    return Cd


@pytest.mark.parametrize("kgroups", gc.BATCHED_KGROUPS)
def test_gemm_batched_gen_exact(kgroups):
    """The general batched kernel with 1, 2 and 4 k-groups per tile ("gemm_kgroups"): the four transposes, 128-bit and
    element-wise loads, accumulation into C, bias and ReLU; 1 .. 7 k-slabs, so groups without a slab occur."""
    la, lib = _la()
    bad = []
    la.check(lib.aomarl_set_option(None, b"gemm_kgroups", kgroups))
    try:
        for c in gc.batched_cases(kgroups):
            d = gc.batched_data(c)
            Cd = _run_batched(c, d)
            want = _dev(d["want"])
            if not torch.equal(Cd, want):
                bad.append("%s: %s" % (_brief(c), _explain(Cd, want, c["M"], c["N"])))
    finally:
        la.check(lib.aomarl_set_option(None, b"gemm_kgroups", 0))
    _report(bad)


# ------------------------------------------------------------------------------------------------ rounding quality
def _ratio(got, want64, bound):
    return float(((got.double().cpu() - want64).abs() / bound).max())


def _pow2_scale(x):
    return 2.0 ** int(np.floor(np.log2(4096.0 / float(np.abs(x).max()))))


@pytest.mark.parametrize("family", ["k_gemm_p", "k_gemm_nt", "k_gemm_nt_h", "k_gemm_g", "k_gemm_batched_gen"])
def test_rounding_quality(family):
    """Heavy-tailed operands (entries over six decades) at each family's forced extremes -- smallest and largest tile,
    one chunk and five, one k-group and four: |err| <= (K + 4) 2^-24 (|alpha| sum |a||b| + |beta C0|), the a-priori
    bound of any order of fp32 summation.  Derived, not tuned: detection is the exact tier's job."""
    la, lib = _la()
    M, N, K = 152, 132, 419
    a = gc.heavy_tailed((M, K), 1)
    b = gc.heavy_tailed((N, K), 2, scale=3e-4)
    c0 = gc.heavy_tailed((M, N), 3)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    absprod = torch.from_numpy(np.abs(a64) @ np.abs(b64).T)
    prod = torch.from_numpy(a64 @ b64.T)
    worst = 0.0
    if family in ("k_gemm_p", "k_gemm_nt", "k_gemm_nt_h"):
        alpha, beta = 0.5, 2.0
        want = alpha * prod + beta * torch.from_numpy(c0.astype(np.float64))
        bound = torch.from_numpy(gc.rounding_bound(K, absprod.numpy(), alpha, beta * c0.astype(np.float64)))
        c = dict(M=M, N=N, K=K, alpha=alpha, beta=beta)
        d = dict(A=gc.padded(a, gc.roundup4(K)), B=gc.padded(b, gc.roundup4(K)), lda=gc.roundup4(K), ldb=gc.roundup4(K),
                 ldc=N, Cbuf=c0, want=c0)
        call = NtCall(c, d)
        kernel = {"k_gemm_p": 1, "k_gemm_nt": 2, "k_gemm_nt_h": 3}[family]
        extra = dict(sa=_pow2_scale(a), sb=_pow2_scale(b)) if kernel == 3 else {}
        la.gemm_saturated(_stream())
        for tile in (((2, 2), (4, 4)) if kernel == 1 else ((0, 0),)):
            for ksplit in (1, 5):
                Cd, _, pr = call.run(kernel=kernel, wm=tile[0], wn=tile[1], ksplit=ksplit, **extra)
                assert pr.r_kernel == kernel and pr.r_nz == ksplit
                worst = max(worst, _ratio(Cd, want, bound))
        assert la.gemm_saturated(_stream()) == 0
    else:
        bound = torch.from_numpy(gc.rounding_bound(K, absprod.numpy()))
        G = 2
        a3, b3 = np.stack([a, a[::-1]]), np.stack([b, b[::-1]])                       # opA(A) [G][M][K], B as [G][N][K]
        want = torch.from_numpy(np.stack([a3[g].astype(np.float64) @ b3[g].astype(np.float64).T for g in range(G)]))
        bound = torch.stack([bound, torch.flip(bound, (0, 1))])
        Mp, Np, Kp = gc.roundup4(M), gc.roundup4(N), gc.roundup4(K)
        forms = {(1, 1): (gc.padded(a3, Kp), gc.padded(b3, Kp)),
                 (1, 0): (gc.padded(a3, Kp), gc.padded(b3.transpose(0, 2, 1), Np)),
                 (0, 1): (gc.padded(a3.transpose(0, 2, 1), Mp), gc.padded(b3, Kp)),
                 (0, 0): (gc.padded(a3.transpose(0, 2, 1), Mp), gc.padded(b3.transpose(0, 2, 1), Np))}
        try:
            for (ak, bk), (An, Bn) in forms.items():
                A, B = _dev(An), _dev(Bn)
                for ext in ((2, 4) if family == "k_gemm_g" else (1, 4)):
                    Cd = torch.full((G, M, N), float("nan"), device="cuda")
                    if family == "k_gemm_g":
                        g = la.GemmGArgs(groups=G, ak=ak, bk=bk, M=M, N=N, K=K, A=A.data_ptr(), lda=An.shape[2],
                                         sA=An.shape[1] * An.shape[2], B=B.data_ptr(), ldb=Bn.shape[2],
                                         sB=Bn.shape[1] * Bn.shape[2], C=Cd.data_ptr(), ldc=N, sC=M * N, force_wm=ext,
                                         force_wn=ext)
                        la.check(lib.aomarl_gemm_g_probe(C.byref(g), _stream()))
                    else:
                        la.check(lib.aomarl_set_option(None, b"gemm_kgroups", ext))
                        la.check(lib.aomarl_gemm_batched(G, 1 - ak, 1 - bk, M, N, K, A.data_ptr(), An.shape[2],
                                                         An.shape[1] * An.shape[2], B.data_ptr(), Bn.shape[2],
                                                         Bn.shape[1] * Bn.shape[2], None, 0, Cd.data_ptr(), N, M * N, 0, 0,
                                                         _stream()))
                    worst = max(worst, _ratio(Cd, want, bound))
        finally:
            la.check(lib.aomarl_set_option(None, b"gemm_kgroups", 0))
    print("rounding quality %s: largest |err| / bound = %.4f" % (family, worst))
    assert worst <= 1.0
