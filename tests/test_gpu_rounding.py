"""-m gpu: the conv / linear kernels, route by route, against correctly rounded float64 references (tests/numerics.py).

Each case names the kernel family that must serve it, forces it with the library's switches (env_switches), confirms it from the launch
profiler (eegldm_prof_dump: class, M / N / K, taps, split-K and the kernel family; the thin direct kernels launch no profiled GEMM) and
holds the result to check A (hard bound: one rounding of an fp32 accumulation in any order) and, for 16-bit outputs, check B (mismatch
share against the fp32 CPU emulation, mean signed ulp error).  Shapes sit at the route edges: sample boundaries inside tiles (L = 96,
192), partial N tiles (192 columns), K tails, the smallest problem a size-gated route accepts and one just below it (which must fall back
to the general kernel and still pass).  Further: fp16 outputs that overflow must be inf and subnormal outputs must equal RNE(ref); a NaN
or inf in an operand must reach every output it feeds; the grouped weight gradient of the UNet backward must equal the per-layer one;
NaN log-variance / x0 must stay NaN through kl_reparam and the sampler steps' clip (as torch.clamp keeps it).

Every case prints one `[numerics]` report line: route, element count, reduction length, worst error in units of its bound
(0.5 ulp + gamma_n * mag for 16-bit outputs, gamma_n * mag for fp32), and for 16-bit outputs the share of elements that differ from
RNE(ref) against the emulation's share and the mean signed ulp error."""
import csv
import math
import os
import tempfile

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

FMT = {0: "f32", 1: "bf16", 2: "f16"}


def _G():
    import gpu_util as G
    return G


def _prof_rows(G, c):
    path = os.path.join(tempfile.gettempdir(), f"eegldm_rounding_rows_{os.getpid()}.csv")
    G.check(G.lib.eegldm_prof_dump(c.h, path.encode()))
    with open(path) as fh:
        return list(csv.DictReader(fh))


def _confirm(rows, want, route):
    """want: None (thin direct kernels: no profiled launch) or dict(kernel=..., cls=..., M=.., N=.., K=.., taps=.., splitk=(lambda s: ..))"""
    seen = [(r["kernel"], int(r["class"]), int(r["M"]), int(r["N"]), int(r["K"]), int(r["taps"]), int(r["splitk"])) for r in rows]
    if want is None:
        assert not seen, f"{route}: expected the thin direct kernels, profiler saw {seen}"
        print(f"[route] {route}: thin direct kernel (no profiled GEMM launch)")
        return
    assert len(seen) == 1, f"{route}: expected one profiled launch, saw {seen}"
    k, cls, M, Nn, K, taps, sk = seen[0]
    assert k == want["kernel"], f"{route}: served by {k}, expected {want['kernel']} ({seen[0]})"
    for name, v in (("cls", cls), ("M", M), ("N", Nn), ("K", K), ("taps", taps)):
        if name in want:
            assert v == want[name], f"{route}: {name} = {v}, expected {want[name]} ({seen[0]})"
    if "splitk" in want:
        assert want["splitk"](sk), f"{route}: splitk = {sk} ({seen[0]})"
    print(f"[route] {route}: {k} class={cls} M={M} N={Nn} K={K} taps={taps} splitk={sk}")


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _poison(t, spots):
    t = t.clone()
    for idx, v in spots:
        t[idx] = v
    return t


# ---------------------------------------------------------------------------------------------------------------- forward
# name, (B, L, Cin, Cout, K, stride, pad_l, pad_r), dtypes, epilogue (b = bias, r = rowvec, s = residual, i = in place), env, pack, expected route
#   pack: "kblk" (eegldm_conv1d_pack_kblocked), "s2" (eegldm_conv1d_pack_stride2)
#   expected: None (thin) or (kernel, M-override or None)
FWD_CASES = [
    ("thin direct k3", (2, 64, 3, 32, 3, 1, 1, 1), (0, 1, 2), "bs", {}, None, None),
    ("thin direct k3 stride2 32->1 (thin_out kernel)", (2, 64, 32, 1, 3, 2, 1, 1), (0, 1, 2), "b", {}, None, None),
    ("conv_skinny 3-tap", (2, 96, 64, 192, 3, 1, 1, 1), (1, 2), "brs", {}, None, "conv_skinny"),
    ("conv_skinny 1x1", (2, 96, 64, 192, 1, 1, 0, 0), (1, 2), "brs", {}, None, "conv_skinny"),
    ("conv_ws Cin128 M16512 (smallest accepted)", (86, 192, 128, 256, 3, 1, 1, 1), (1, 2), "brs", {}, None, "conv_ws"),
    ("conv_ws M16320 (one sample below: general kernel)", (85, 192, 128, 256, 3, 1, 1, 1), (1,), "brs", {}, None, "gemm"),
    ("conv_ws2 stride2 128->256 M8192", (64, 256, 128, 256, 3, 2, 1, 1), (1, 2), "b", {}, None, "conv_ws2"),
    ("conv_ws paired rows stride2 64->128", (128, 256, 64, 128, 3, 2, 1, 1), (1, 2), "b", {}, "s2", "conv_ws"),
    ("gemm 128x128 3-tap partial N tile", (2, 192, 128, 192, 3, 1, 1, 1), (0, 1, 2), "brs", {"EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm"),
    ("gemm 128x128 3-tap K-blocked", (2, 192, 128, 192, 3, 1, 1, 1), (1, 2), "brs", {"EEGLDM_NO_CONV_SKINNY": "1"}, "kblk", "gemm_kblk"),
    ("gemm 128x128 1x1 K tail 160", (2, 40, 160, 32, 1, 1, 0, 0), (0, 1), "b", {"EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm"),
    ("gemm stride2 right pad only", (2, 128, 32, 32, 3, 2, 0, 1), (0, 1, 2), "b", {}, None, "gemm"),
    ("gemm_big 3-tap persistent", (2, 384, 256, 256, 3, 1, 1, 1), (1, 2), "brs", {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, "kblk", "gemm_big"),
    ("gemm_big 3-tap one tile per workgroup", (2, 384, 256, 256, 3, 1, 1, 1), (1,), "brs",
     {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_GEMM_BIG_NO_PERSIST": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, "kblk", "gemm_big"),
    ("gemm_big 3-tap in-place residual", (2, 384, 256, 256, 3, 1, 1, 1), (1, 2), "brsi", {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, "kblk", "gemm_big"),
    ("gemm_big 3-tap plain weights, 8 tiles = min", (2, 384, 256, 512, 3, 1, 1, 1), (1,), "b",
     {"EEGLDM_GEMM_BIG_MIN_TILES": "8", "EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm_big"),
    ("gemm_big below min tiles -> gemm", (2, 384, 256, 512, 3, 1, 1, 1), (1,), "b",
     {"EEGLDM_GEMM_BIG_MIN_TILES": "9", "EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm"),
    ("gemm_big 1x1 persistent", (2, 384, 512, 256, 1, 1, 0, 0), (1, 2), "brs", {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm_big"),
    ("gemm_big 1x1 one tile per workgroup", (2, 384, 512, 256, 1, 1, 0, 0), (1,), "brs",
     {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_GEMM_BIG1_NO_PERSIST": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm_big"),
    ("gemm 1x1 with big 1x1 off", (2, 384, 512, 256, 1, 1, 0, 0), (1,), "brs",
     {"EEGLDM_GEMM_BIG_MIN_TILES": "1", "EEGLDM_NO_GEMM_BIG1": "1", "EEGLDM_NO_CONV_SKINNY": "1"}, None, "gemm"),
]


def _fwd_case(G, c, case, dt, env_switches, scale=1.0, poison=False, report_tag=""):
    name, (B, L, Cin, Cout, K, s, pl, pr), _dts, ep, env, pack, want = case
    fmt = FMT[dt]
    env_switches(**env)
    x = N.to_storage(_randn((B, Cin, L), 1), fmt)
    w = N.to_storage(_randn((Cout, Cin, K), 2, scale / math.sqrt(Cin * K)), fmt)
    if poison:
        x = _poison(x, [((1, min(5, Cin - 1), 7), math.nan), ((0, Cin - 1, L // 2), math.inf)])
    Lout = (L + pl + pr - K) // s + 1
    b = N.rne(_randn((Cout,), 3, scale), "f32") if "b" in ep else None
    row = N.rne(_randn((B, Cout), 4, scale), "f32") if "r" in ep else None
    res = N.to_storage(_randn((B, Cout, Lout), 5, scale), fmt) if "s" in ep else None
    ref, mag, emul = N.evaluate(N.conv1d_fwd, x, w, b, s, pl, pr, row, res)
    if fmt == "f16" and scale > 1:          # the range cases must reach their range, or they test nothing
        assert float(torch.isinf(N.rne(ref, "f16")).double().mean()) > 1e-3, f"{name}: no output overflows fp16 at scale {scale}"
    if fmt == "f16" and scale < 1:
        r16 = N.rne(ref, "f16")
        assert float(((r16 != 0) & (r16.abs() < 2.0 ** -14)).double().mean()) > 0.5, f"{name}: outputs not in the fp16 subnormal range"
    if poison and pack == "s2":
        # paired-row route (ops.hip): y[t] is a 3-tap conv over the row pairs t - 1, t, t + 1 = input rows 2t - 2 .. 2t + 3, zero taps on
        # rows 2t - 2, 2t + 2, 2t + 3: a non-finite x[r] turns every y[t] with 2t - 2 <= r <= 2t + 3 NaN (the reference: 2t - 1 <= r <= 2t + 1)
        for bi, r in ((1, 7), (0, L // 2)):
            for t in range(Lout):
                if 2 * t - 2 <= r <= 2 * t + 3:
                    ref[bi, :, t] = torch.where(torch.isfinite(ref[bi, :, t]), math.nan, ref[bi, :, t])
    xd, wd = G.nlc(x, dt), G.pack_w(w, dt)
    bd = b.float().to(G.DEV) if b is not None else None
    rd = row.float().to(G.DEV).contiguous() if row is not None else None
    sd = G.nlc(res, dt) if res is not None else None
    yd = sd.clone() if "i" in ep else torch.full((B * Lout, Cout), float("nan"), device=G.DEV, dtype=G.TDT[dt])
    keep = []
    if pack == "kblk":
        keep.append(torch.empty_like(wd)); G.check(G.lib.eegldm_conv1d_pack_kblocked_k(c.h, G.ptr(wd), G.ptr(keep[-1]), Cout, Cin, K, dt))
    elif pack == "s2":
        keep += [torch.empty(3 * 128 * 128, device=G.DEV, dtype=G.TDT[dt]) for _ in range(2)]
        G.check(G.lib.eegldm_conv1d_pack_stride2(c.h, G.ptr(wd), G.ptr(keep[0]), G.ptr(keep[1]), Cout, Cin, dt))
    try:
        c.prof_enable(True)
        G.check(G.lib.eegldm_conv1d_fwd(c.h, G.ptr(xd), Cin, G.ptr(wd), G.ptr(bd) if bd is not None else None, G.ptr(yd), Cout, B, L, Cin, Cout, K, s, pl, pr,
                                        G.ptr(rd) if rd is not None else None, Cout if rd is not None else 0,
                                        G.ptr(yd if "i" in ep else sd) if sd is not None else None, Cout if sd is not None else 0, dt))
        torch.cuda.synchronize()
        rows = _prof_rows(G, c)
    finally:
        c.prof_enable(False)
        if pack:
            G.check(G.lib.eegldm_conv1d_forget_kblocked(c.h, G.ptr(wd)))
    route = f"fwd {name}{report_tag}"
    if want is None:
        _confirm(rows, None, route)
    elif want == "conv_ws" and pack == "s2":
        _confirm(rows, dict(kernel="conv_ws", cls=0, M=B * Lout, N=128, K=128, taps=3), route)
    else:
        _confirm(rows, dict(kernel=want, cls=0 if K == 3 else 3, M=B * Lout, N=Cout, K=Cin, taps=K), route)
    return N.check(G.ncl(yd, B, Lout), ref, mag, K * Cin, fmt, emul=emul, route=route)


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward_route(case, env_switches):
    G = _G(); c = G.ctx()
    for dt in case[2]:
        _fwd_case(G, c, case, dt, env_switches)


FWD_EDGE = [c for c in FWD_CASES if c[0] in ("thin direct k3", "conv_skinny 3-tap", "conv_ws Cin128 M16512 (smallest accepted)", "gemm 128x128 3-tap partial N tile",
                                              "gemm_big 3-tap persistent", "gemm_big 1x1 persistent", "conv_ws2 stride2 128->256 M8192",
                                              "conv_ws paired rows stride2 64->128")]


@pytest.mark.parametrize("case", FWD_EDGE, ids=[c[0] for c in FWD_EDGE])
def test_forward_fp16_range_and_nonfinite(case, env_switches):
    """fp16: outputs whose RNE(ref) overflows must be inf (not 65504), outputs in the subnormal range must equal RNE(ref) (not 0); with a NaN
    and an inf in x every output they feed must be NaN / inf as in the reference (f16, and bf16 for the non-finite inputs)"""
    G = _G(); c = G.ctx()
    _fwd_case(G, c, case, 2, env_switches, scale=2.0 ** 15, report_tag=" [f16 overflow range]")
    _fwd_case(G, c, case, 2, env_switches, scale=2.0 ** -17, report_tag=" [f16 subnormal range]")
    for dt in (1, 2):
        _fwd_case(G, c, case, dt, env_switches, poison=True, report_tag=" [NaN/inf in x]")


SKIP_CASES = [(2, 192, 256, 128, 256, 1), (2, 384, 256, 256, 256, 0)]     # B, L, Cmid, Cin2, Cout, rowvec


@pytest.mark.parametrize("case", SKIP_CASES)
def test_skip_fwd_fused_launch(case, env_switches):
    """eegldm_conv1d_skip_fwd on the big tile: conv3(h) + b + conv1(x2) + b2 (+ row) with one fp32 accumulator and ONE rounding"""
    G = _G(); c = G.ctx()
    B, L, Cm, C2, Co, rv = case
    env_switches(EEGLDM_GEMM_BIG_MIN_TILES="1")
    for dt in (1, 2):
        fmt = FMT[dt]
        h = N.to_storage(_randn((B, Cm, L), 11), fmt); x2 = N.to_storage(_randn((B, C2, L), 12), fmt)
        w = N.to_storage(_randn((Co, Cm, 3), 13, 1 / math.sqrt(3 * Cm)), fmt); w2 = N.to_storage(_randn((Co, C2, 1), 14, 1 / math.sqrt(C2)), fmt)
        b, b2 = N.rne(_randn((Co,), 15), "f32"), N.rne(_randn((Co,), 16), "f32")
        row = N.rne(_randn((B, Co), 17), "f32") if rv else None
        fn = lambda h, w, b, x2, w2, b2, row: N.conv1d_fwd(h, w, b, 1, 1, 1, row) + N.conv1d_fwd(x2, w2, b2)
        ref, mag, emul = N.evaluate(fn, h, w, b, x2, w2, b2, row)
        hd, xd, wd, w2d = G.nlc(h, dt), G.nlc(x2, dt), G.pack_w(w, dt), G.pack_w(w2, dt)
        bd, b2d = b.float().to(G.DEV), b2.float().to(G.DEV); rd = row.float().to(G.DEV) if rv else None
        wk, w2k = torch.empty_like(wd), torch.empty_like(w2d)
        G.check(G.lib.eegldm_conv1d_pack_kblocked(c.h, G.ptr(wd), G.ptr(wk), Co, Cm, dt))
        G.check(G.lib.eegldm_conv1d_pack_kblocked_k(c.h, G.ptr(w2d), G.ptr(w2k), Co, C2, 1, dt))
        yd = torch.full((B * L, Co), float("nan"), device=G.DEV, dtype=G.TDT[dt])
        try:
            c.prof_enable(True)
            G.check(G.lib.eegldm_conv1d_skip_fwd(c.h, G.ptr(hd), Cm, G.ptr(wd), G.ptr(bd), G.ptr(xd), C2, G.ptr(w2d), G.ptr(b2d), G.ptr(yd), Co,
                                                 B, L, Cm, C2, Co, G.ptr(rd) if rv else None, Co if rv else 0, dt))
            rows = _prof_rows(G, c)
        finally:
            c.prof_enable(False)
            G.check(G.lib.eegldm_conv1d_forget_kblocked(c.h, G.ptr(wd))); G.check(G.lib.eegldm_conv1d_forget_kblocked(c.h, G.ptr(w2d)))
        route = f"skip_fwd {B}x{L} {Cm}+{C2}->{Co}"
        _confirm(rows, dict(kernel="gemm_big_skip", cls=0, M=B * L, N=Co, taps=3), route)
        N.check(G.ncl(yd, B, L), ref, mag, 3 * Cm + C2, fmt, emul=emul, route=route)


# ---------------------------------------------------------------------------------------------------------------- data gradient
# name, (B, L, Cin, Cout, K, stride, pad_l, pad_r), dtypes, residual, env, pack ("dgrad_k", "s2"), expected
DGRAD_CASES = [
    ("thin direct", (2, 64, 3, 32, 3, 1, 1, 1), (0, 1, 2), False, {}, None, None),
    ("gemm transposed 3-tap partial N tile", (2, 192, 192, 128, 3, 1, 1, 1), (0, 1, 2), True, {}, None, "gemm"),
    ("gemm transposed stride2", (2, 128, 64, 128, 3, 2, 1, 1), (0, 1, 2), False, {}, None, "gemm"),
    ("gemm transposed 1x1", (2, 96, 64, 192, 1, 1, 0, 0), (0, 1), True, {}, None, "gemm"),
    ("gemm_big NT on the pack_dgrad_k copy 3-tap", (2, 384, 256, 256, 3, 1, 1, 1), (1, 2), True, {"EEGLDM_GEMM_BIG_MIN_TILES": "1"}, "dgrad_k", "gemm_big"),
    ("gemm_big NT on the pack_dgrad_k copy 1x1", (2, 384, 256, 256, 1, 1, 0, 0), (1, 2), False, {"EEGLDM_GEMM_BIG_MIN_TILES": "1"}, "dgrad_k", "gemm_big"),
    ("conv_ws transposed (Cout 128, M16512)", (86, 192, 256, 128, 3, 1, 1, 1), (1, 2), True, {}, None, "conv_ws"),
    ("conv_ws2 stride2 data gradient", (64, 256, 128, 256, 3, 2, 1, 1), (1, 2), False, {}, None, "conv_ws2"),
    ("conv_ws paired rows stride2 64->128 data gradient", (128, 256, 64, 128, 3, 2, 1, 1), (1,), False, {}, "s2", "conv_ws"),
]


def _dgrad_case(G, c, case, dt, env_switches, poison=False):
    name, (B, L, Cin, Cout, K, s, pl, pr), _dts, rs, env, pack, want = case
    fmt = FMT[dt]
    env_switches(**env)
    Lout = (L + pl + pr - K) // s + 1
    w = N.to_storage(_randn((Cout, Cin, K), 21, 1 / math.sqrt(Cout * K)), fmt)
    dy = N.to_storage(_randn((B, Cout, Lout), 22), fmt)
    if poison:
        dy = _poison(dy, [((1, min(3, Cout - 1), Lout // 2), math.nan), ((0, Cout - 1, 0), -math.inf)])
    res = N.to_storage(_randn((B, Cin, L), 23), fmt) if rs else None
    ref, mag, emul = N.evaluate(N.conv1d_dgrad, dy, w, L, s, pl, pr, res)
    if poison and pack == "s2":
        # paired-row route (ops.hip): dy row t feeds the dx row PAIRS t - 1, t, t + 1 (zero taps included): those rows turn NaN
        for bi, t in ((1, Lout // 2), (0, 0)):
            for pp in (t - 1, t, t + 1):
                if 0 <= pp < Lout:
                    ref[bi, :, 2 * pp:2 * pp + 2] = torch.where(torch.isfinite(ref[bi, :, 2 * pp:2 * pp + 2]), math.nan, ref[bi, :, 2 * pp:2 * pp + 2])
    dyd, wd = G.nlc(dy, dt), G.pack_w(w, dt)
    rd = G.nlc(res, dt) if rs else None
    dxd = torch.full((B * L, Cin), float("nan"), device=G.DEV, dtype=G.TDT[dt])
    keep = []
    if pack == "dgrad_k":
        keep.append(torch.empty_like(wd)); G.check(G.lib.eegldm_conv1d_pack_dgrad_k(c.h, G.ptr(wd), G.ptr(keep[0]), Cout, Cin, K, dt))
    elif pack == "s2":
        keep += [torch.empty(3 * 128 * 128, device=G.DEV, dtype=G.TDT[dt]) for _ in range(2)]
        G.check(G.lib.eegldm_conv1d_pack_stride2(c.h, G.ptr(wd), G.ptr(keep[0]), G.ptr(keep[1]), Cout, Cin, dt))
    try:
        c.prof_enable(True)
        G.check(G.lib.eegldm_conv1d_bwd_data(c.h, G.ptr(dyd), Cout, G.ptr(wd), G.ptr(dxd), Cin, B, L, Cin, Cout, K, s, pl, pr,
                                             G.ptr(rd) if rs else None, Cin if rs else 0, dt))
        torch.cuda.synchronize()
        rows = _prof_rows(G, c)
    finally:
        c.prof_enable(False)
        if pack:
            G.check(G.lib.eegldm_conv1d_forget_kblocked(c.h, G.ptr(wd)))
    route = f"dgrad {name}" + (" [NaN/inf in dy]" if poison else "")
    if want is None:
        _confirm(rows, None, route)
    elif want == "conv_ws2":
        _confirm(rows, dict(kernel="conv_ws2", cls=1, M=B * Lout, N=256, K=128, taps=3), route)
    elif pack == "s2":
        _confirm(rows, dict(kernel="conv_ws", cls=0, M=B * Lout, N=128, K=128, taps=3), route)
    elif want == "gemm" and K == 1:
        _confirm(rows, dict(kernel="gemm", M=B * L, N=Cin, K=Cout, taps=1), route)
    else:
        _confirm(rows, dict(kernel=want, M=B * L, N=Cin, K=Cout, taps=K), route)
    return N.check(G.ncl(dxd, B, L), ref, mag, K * Cout, fmt, emul=emul, route=route)


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_data_gradient_route(case, env_switches):
    G = _G(); c = G.ctx()
    for dt in case[2]:
        _dgrad_case(G, c, case, dt, env_switches)
    _dgrad_case(G, c, case, case[2][-1], env_switches, poison=True)


# ---------------------------------------------------------------------------------------------------------------- weight + bias gradient
# name, (B, L, Cin, Cout, K, stride, pad_l, pad_r), dtypes, env, expected kernel, expected taps in the record, split-K expected
WGRAD_CASES = [
    ("fused 3-tap split-K", (8, 192, 128, 192, 3, 1, 1, 1), (0, 1, 2), {}, "gemm_splitk_fold", 3, True),
    ("fused 3-tap, bias by the column-sum kernel", (8, 192, 128, 192, 3, 1, 1, 1), (1,), {"EEGLDM_NO_FUSED_BIAS_GRAD": "1"}, "gemm_splitk_fold", 3, True),
    ("fused 3-tap deterministic", (8, 192, 128, 192, 3, 1, 1, 1), (1, 2), {"EEGLDM_DETERMINISTIC": "1"}, "gemm_splitk_fold", 3, True),
    # by-tap: K splits drain through fp32 atomics ("gemm", splitk > 1); in the deterministic mode through written partials + fold
    ("by-tap (L = 80: no whole K stages per sample)", (16, 80, 128, 192, 3, 1, 1, 1), (0, 1, 2), {}, "gemm", 3, True),
    ("by-tap stride2", (2, 128, 64, 128, 3, 2, 1, 1), (0, 1), {}, "gemm", 3, None),
    ("by-tap deterministic", (16, 80, 128, 192, 3, 1, 1, 1), (1, 2), {"EEGLDM_DETERMINISTIC": "1"}, "gemm_splitk_fold", 3, True),
    ("1x1 TN split-K", (8, 192, 256, 192, 1, 1, 0, 0), (0, 1, 2), {}, "gemm_splitk_fold", 1, True),
    ("thin dconv_wgrad", (2, 64, 3, 32, 3, 1, 1, 1), (0, 1, 2), {}, None, None, None),
    ("thin dconv_wgrad conv_out shape", (2, 64, 32, 1, 3, 1, 1, 1), (0, 1), {}, None, None, None),
]


def _wgrad_case(G, c, case, dt, env_switches, accumulate=False, poison=False):
    name, (B, L, Cin, Cout, K, s, pl, pr), _dts, env, want, taps, split = case
    fmt = FMT[dt]
    env_switches(**env)
    Lout = (L + pl + pr - K) // s + 1
    x = N.to_storage(_randn((B, Cin, L), 31), fmt)
    dy = N.to_storage(_randn((B, Cout, Lout), 32), fmt)
    if poison:
        dy = _poison(dy, [((1, min(3, Cout - 1), Lout // 2), math.nan), ((0, Cout - 1, 1), math.inf)])
    acc_w = N.rne(_randn((Cout, Cin, K), 33, 8.0), "f32") if accumulate else None
    acc_b = N.rne(_randn((Cout,), 34, 8.0), "f32") if accumulate else None
    ref, mag, _ = N.evaluate(N.conv1d_wgrad, x, dy, K, s, pl, pr, acc_w)
    bref, bmag, _ = N.evaluate(N.bias_grad, dy, acc_b)
    xd, dyd = G.nlc(x, dt), G.nlc(dy, dt)
    dwd = G.pack_w(acc_w.float(), 0) if accumulate else torch.zeros(K, Cout, Cin, device=G.DEV)
    dbd = acc_b.float().to(G.DEV) if accumulate else torch.zeros(Cout, device=G.DEV)
    try:
        c.prof_enable(True)
        G.check(G.lib.eegldm_conv1d_bwd_weight(c.h, G.ptr(xd), Cin, G.ptr(dyd), Cout, G.ptr(dwd), G.ptr(dbd), B, L, Cin, Cout, K, s, pl, pr, dt))
        torch.cuda.synchronize()
        rows = _prof_rows(G, c)
    finally:
        c.prof_enable(False)
    route = f"wgrad {name}" + (" [+= non-zero]" if accumulate else "") + (" [NaN/inf in dy]" if poison else "")
    if taps is None:
        _confirm(rows, None, route)
    else:
        w_ = dict(kernel=want, cls=2 if K == 3 else 5, M=Cout, N=Cin, K=B * Lout, taps=taps)
        if split:
            w_["splitk"] = lambda sk: sk > 1
        _confirm(rows, w_, route)
    n = B * Lout
    N.check(G.unpack_w(dwd), ref, mag, n, "f32", route=route + " dW")
    N.check(dbd.cpu(), bref, bmag, n, "f32", route=route + " db")
    if poison:
        flag = torch.zeros(1, device=G.DEV)
        G.check(G.lib.eegldm_grad_check_finite(c.h, G.ptr(dwd), dwd.numel(), G.ptr(flag)))
        assert float(flag) == 1.0, f"{route}: eegldm_grad_check_finite missed the non-finite dW"
    return dwd, dbd


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_weight_gradient_route(case, env_switches):
    G = _G(); c = G.ctx()
    for dt in case[2]:
        dw, db = _wgrad_case(G, c, case, dt, env_switches)
        if case[3].get("EEGLDM_DETERMINISTIC"):         # the deterministic mode: a second launch reproduces dW and db bit for bit
            dw2, db2 = _wgrad_case(G, c, case, dt, env_switches)
            assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32)), case[0]
    _wgrad_case(G, c, case, case[2][-1], env_switches, accumulate=True)
    _wgrad_case(G, c, case, case[2][-1], env_switches, poison=True)


# ---------------------------------------------------------------------------------------------------------------- linear
LINEAR_CASES = [(8, 512, 128), (256, 512, 512), (256, 7168, 512), (5, 96, 40), (3, 8, 32)]     # M, N, K (test_gpu_primitives.py)


@pytest.mark.parametrize("case", LINEAR_CASES)
def test_linear_fwd_bwd(case):
    """nn.Linear forward (fp32 out), dx (fp32 out), dW += and db += (fp32), for fp32 and bf16 operands; the serving kernels are reported"""
    G = _G(); c = G.ctx()
    M, Nn, K = case
    for dt in (0, 1):
        fmt = FMT[dt]
        x = N.to_storage(_randn((M, K), 41), fmt); w = N.to_storage(_randn((Nn, K), 42, 1 / math.sqrt(K)), fmt)
        b = N.rne(_randn((Nn,), 43), "f32"); dy = N.to_storage(_randn((M, Nn), 44), fmt)
        acc = N.rne(_randn((Nn, K), 45, 4.0), "f32")
        yr, ym, _ = N.evaluate(N.linear_fwd, x, w, b)
        dxr, dxm, _ = N.evaluate(N.linear_dgrad, dy, w)
        dwr, dwm, _ = N.evaluate(N.linear_wgrad, x, dy, acc)
        dbr, dbm, _ = N.evaluate(N.bias_grad, dy)
        td = G.TDT[dt]
        xd, wd, bd, dyd = x.to(G.DEV).to(td), w.to(G.DEV).to(td), b.float().to(G.DEV), dy.to(G.DEV).to(td)
        yd = torch.empty(M, Nn, device=G.DEV); dxd = torch.empty(M, K, device=G.DEV)
        dwd = acc.float().to(G.DEV).contiguous(); dbd = torch.zeros(Nn, device=G.DEV)
        c.prof_enable(True)
        try:
            G.check(G.lib.eegldm_linear_fwd(c.h, G.ptr(xd), K, G.ptr(wd), G.ptr(bd), G.ptr(yd), Nn, M, Nn, K, dt, 1))
            G.check(G.lib.eegldm_linear_bwd(c.h, G.ptr(xd), K, G.ptr(wd), G.ptr(dyd), Nn, G.ptr(dxd), K, G.ptr(dwd), G.ptr(dbd), M, Nn, K, dt, 1))
            rows = _prof_rows(G, c)
        finally:
            c.prof_enable(False)
        print(f"[route] linear {case} {fmt}: " + ", ".join(f"{r['kernel']}(class {r['class']} M={r['M']} N={r['N']} K={r['K']} splitk={r['splitk']})" for r in rows))
        N.check(yd, yr, ym, K, "f32", route=f"linear fwd {case} [{fmt} operands]")
        N.check(dxd, dxr, dxm, Nn, "f32", route=f"linear dx {case} [{fmt} operands]")
        N.check(dwd, dwr, dwm, M, "f32", route=f"linear dW += {case} [{fmt} operands]")
        N.check(dbd, dbr, dbm, M, "f32", route=f"linear db {case} [{fmt} operands]")


# ---------------------------------------------------------------------------------------------------------------- grouped weight gradients
GCFG = dict(in_channels=1, out_channels=1, model_channels=64, num_res_blocks=2, attention_resolutions=[2], channel_mult=[1, 2], resblock_updown=False)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_grouped_weight_gradient_equals_per_layer(dtype, env_switches):
    """The UNet backward records the weight gradients of its GEMM-path convs and launches each group of same-shape layers as ONE grouped
    split-K GEMM (op_wgrad_flush -> gemm_launch_grouped -> splitk_fold_grouped_kernel), and folds the GroupNorm dgamma / dbeta slots in
    batches.  EEGLDM_NO_GROUPED_WGRAD=1 launches one GEMM per layer.  Both in the deterministic mode (fixed-order folds), profiled to
    confirm the routes; and the grouped path once more as training runs it (default mode, no profiling: the profiler serialises the
    streams).  Every parameter gradient must agree with the per-layer one to fp32 reordering noise (rel-L2 <= 1e-5 per tensor; the default
    mode adds the ~2e-7 atomic-order spread) and exact zeros must agree."""
    from eegldm.models import UNetModel
    from param_gen import gen_param
    G = _G()
    B, L = 8, 384
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, 1, L, generator=g).cuda(); t = torch.randint(0, 1000, (B,), generator=g).cuda(); dy = torch.randn(B, 1, L, generator=g).cuda()
    out = {}
    for mode, sw, det, prof in (("grouped", None, "1", True), ("per-layer", "1", "1", True), ("grouped, training mode", None, None, False)):
        env_switches(EEGLDM_NO_GROUPED_WGRAD=sw, EEGLDM_DETERMINISTIC=det)
        net = UNetModel(image_size=L, dtype=dtype, **GCFG)
        net.load_state_dict({k: torch.from_numpy(gen_param(5, k, tuple(v.shape))) for k, v in net.state_dict().items()})
        net.train(); net.zero_grad()
        net._forward_native(x, t)
        net.ctx.prof_enable(prof)
        try:
            net.backward(dy)
            torch.cuda.synchronize()
            rows = _prof_rows(G, net.ctx) if prof else []
        finally:
            net.ctx.prof_enable(False)
        kinds = {}
        for r in rows:
            kinds[r["kernel"]] = kinds.get(r["kernel"], 0) + 1
        print(f"[route] UNet backward {dtype} {mode}: {kinds}")
        out[mode] = ({k: v.detach().cpu().double().clone() for k, v in net.grad_dict().items()}, kinds)
    assert out["grouped"][1].get("gemm_grouped", 0) >= 1, out["grouped"][1]
    assert out["per-layer"][1].get("gemm_grouped", 0) == 0, out["per-layer"][1]
    gb = out["per-layer"][0]
    for mode in ("grouped", "grouped, training mode"):
        ga = out[mode][0]
        worst = ("", 0.0)
        for k in gb:
            a, b = ga[k], gb[k]
            assert torch.isfinite(a).all() and torch.isfinite(b).all(), k
            assert torch.equal(a == 0, b == 0), f"{mode} {k}: exact zeros differ ({int(((a == 0) != (b == 0)).sum())} elements)"
            rel = float((a - b).norm() / b.norm()) if float(b.norm()) > 0 else float(a.norm())
            if rel > worst[1]:
                worst = (k, rel)
            assert rel <= 1e-5, f"{mode} {k}: grouped vs per-layer rel-L2 {rel:.3e}"
        print(f"[numerics] {mode} vs per-layer weight gradients {dtype}: {len(gb)} tensors, worst rel-L2 {worst[1]:.2e} ({worst[0]})")


# ---------------------------------------------------------------------------------------------------------------- NaN through the clamps
@pytest.mark.parametrize("dt", [0, 1, 2])
def test_kl_reparam_keeps_nan_log_variance(dt):
    """sigma = exp(clamp(lv, -30, 20) / 2): torch.clamp keeps a NaN, so sigma, z and the KL sum are NaN where lv is; the backward mask
    -30 < lv < 20 is false for NaN (dlv = 0, as torch's clamp backward gives), and a NaN in dz reaches dmu and dlv"""
    G = _G(); c = G.ctx()
    fmt = FMT[dt]; td = G.TDT[dt]
    n, B = 4096, 4
    mu = N.to_storage(_randn((n,), 51), fmt); lv = N.to_storage(_randn((n,), 52, 3.0), fmt)
    lv[[0, 1, 2]] = torch.tensor([-40.0, 25.0, 0.5], dtype=torch.float64)
    lv[7] = math.nan; lv[9] = math.inf
    eps = N.rne(_randn((n,), 53), "f32").float()
    sig_ref = torch.exp(torch.clamp(lv, -30, 20) / 2)
    z_ref = mu + eps.double() * sig_ref
    mud, lvd, epsd = mu.to(G.DEV).to(td), lv.to(G.DEV).to(td), eps.to(G.DEV)
    zd = torch.empty(n, device=G.DEV, dtype=td); sgd = torch.empty(n, device=G.DEV); kl = torch.zeros(1, device=G.DEV)
    G.check(G.lib.eegldm_kl_reparam_fwd(c.h, G.ptr(mud), G.ptr(lvd), G.ptr(epsd), G.ptr(zd), G.ptr(sgd), G.ptr(kl), n, B, dt))
    torch.cuda.synchronize()
    sg, z = sgd.cpu().double(), zd.float().cpu().double()
    assert math.isnan(float(sg[7])) and math.isnan(float(z[7])), (float(sg[7]), float(z[7]))
    assert math.isnan(float(kl)), float(kl)
    fin = torch.isfinite(sig_ref)
    assert torch.allclose(sg[fin], sig_ref[fin], rtol=1e-5, atol=0), "sigma"
    assert abs(float(sg[9]) / math.exp(10.0) - 1) < 1e-5, float(sg[9])          # +inf log-variance clamps to 20
    # backward: NaN in dz at 100 -> dmu[100], dlv[100] NaN; NaN lv at 7 -> dlv[7] = 0
    dz = N.to_storage(_randn((n,), 54), fmt); dz[100] = math.nan
    dzd = dz.to(G.DEV).to(td); dmu = torch.empty(n, device=G.DEV, dtype=td); dlv = torch.empty(n, device=G.DEV, dtype=td)
    G.check(G.lib.eegldm_kl_reparam_bwd(c.h, G.ptr(mud), G.ptr(lvd), G.ptr(epsd), G.ptr(sgd), G.ptr(dzd), G.ptr(dmu), G.ptr(dlv), n, 0.25, dt))
    torch.cuda.synchronize()
    dm, dl = dmu.float().cpu(), dlv.float().cpu()
    assert math.isnan(float(dm[100])) and math.isnan(float(dl[100])), (float(dm[100]), float(dl[100]))
    assert float(dl[7]) == 0.0 and float(dl[0]) == 0.0 and float(dl[1]) == 0.0 and float(dl[9]) == 0.0
    mask = torch.ones(n, dtype=torch.bool); mask[[7, 100]] = False
    assert torch.isfinite(dm[mask]).all() and torch.isfinite(dl[mask]).all()


@pytest.mark.parametrize("step", ["ddim", "ddim_eta", "ddpm"])
def test_sampler_clip_keeps_nan(step):
    """clip_sample: x0 = clamp(x0, -1, 1) keeps a NaN x0 (torch.clamp); before the fix fmaxf turned it into -1 and the step a finite sample"""
    G = _G(); c = G.ctx()
    n = 4096
    mo = _randn((n,), 61).float(); x = _randn((n,), 62, 3.0).float(); nz = _randn((n,), 63).float()
    mo[5] = math.nan; mo[6] = math.inf
    a_t, a_prev, beta = 0.3, 0.5, 0.02
    mod, xd, nzd = mo.to(G.DEV), x.to(G.DEV), nz.to(G.DEV)
    prev = torch.empty(n, device=G.DEV); x0 = torch.empty(n, device=G.DEV)
    if step == "ddim":
        G.check(G.lib.eegldm_ddim_step(c.h, G.ptr(mod), G.ptr(xd), a_t, a_prev, 0, 1, G.ptr(prev), G.ptr(x0), n))
    elif step == "ddim_eta":
        G.check(G.lib.eegldm_ddim_step_eta(c.h, G.ptr(mod), G.ptr(xd), G.ptr(nzd), a_t, a_prev, 0.5, 0, 1, G.ptr(prev), G.ptr(x0), n))
    else:
        G.check(G.lib.eegldm_ddpm_step(c.h, G.ptr(mod), G.ptr(xd), G.ptr(nzd), a_t, a_prev, beta, 0, 1, G.ptr(prev), G.ptr(x0), n))
    torch.cuda.synchronize()
    x0_ref = torch.clamp((x.double() - math.sqrt(1 - a_t) * mo.double()) / math.sqrt(a_t), -1, 1)
    p, q = prev.cpu(), x0.cpu()
    assert math.isnan(float(q[5])) and math.isnan(float(p[5])), (step, float(q[5]), float(p[5]))
    assert float(q[6]) == -1.0                                  # -inf x0 is clamped (finite), as torch does
    m = torch.isfinite(x0_ref)
    assert torch.allclose(q[m].double(), x0_ref[m], rtol=1e-5, atol=1e-6)
    mask = torch.ones(n, dtype=torch.bool); mask[[5, 6]] = False         # (an infinite model output makes prev infinite)
    if step == "ddim":
        assert torch.isfinite(p[mask]).all()


def test_thin_autoencoder_heads_keep_nan_log_variance(env_switches):
    """The whole-network kernels of the [2,2,4] autoencoder (aekl_thin.hip f_heads_t) clamp the log-variance head in registers: a NaN log
    variance must give NaN sigma, z, reconstruction and KL there as on the layer-by-layer path (losses.hip) and in the reference; mu stays
    finite.  (Before the NaN-keeping clamp it became -30: sigma = exp(-15) and a finite z.)"""
    from eegldm.models import AutoencoderKL
    from param_gen import gen_param
    B, L = 2, 3072
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 1, L, generator=g); eps = torch.randn(B, 1, L // 4, generator=g)
    for no_thin in (None, "1"):
        env_switches(EEGLDM_AEKL_NO_THIN=no_thin)
        net = AutoencoderKL(spatial_dims=1, in_channels=1, out_channels=1, num_channels=[2, 2, 4], latent_channels=1, num_res_blocks=2,
                            norm_num_groups=1, attention_levels=[False] * 3, dtype="float32")
        sd = {k: torch.from_numpy(gen_param(4, k, shape)) for k, (_o, _n, shape) in net.entries.items()}
        keys = [k for k in sd if "quant_conv_log_sigma" in k and k.endswith("bias")]
        assert keys, list(sd)
        sd[keys[0]] = torch.full_like(sd[keys[0]], float("nan"))
        net.load_state_dict(sd)
        kl = torch.zeros(1, device=net.device)
        recon, mu, sg = net(x, eps=eps, kl_out=kl)
        torch.cuda.synchronize()
        path = "layer-by-layer" if no_thin else "whole-network kernels"
        assert torch.isfinite(mu).all(), path
        assert torch.isnan(sg).all(), (path, sg.flatten()[:4])
        assert torch.isnan(recon).all(), path
        assert math.isnan(float(kl)), (path, float(kl))


# ---------------------------------------------------------------------------------------------------------------- GroupNorm
# B, L, C, G, silu, mean offset (in units of the standard deviation)
GN_CASES = [(4, 768, 64, 32, 1, 0.0), (4, 768, 64, 32, 1, 30.0), (2, 3072, 8, 1, 1, 0.0), (2, 3072, 8, 1, 1, 30.0), (4, 192, 256, 32, 0, 30.0)]
# Case (4, 192, 256, 32, 0, 30.0) -- mean 30 x std, 8 channels per group, no SiLU, the register-resident kernels -- carried an open finding
# until the one-pass statistics were repaired (norm.hip: sums about a pivot shared by the group, fp64 divisor): fp16 forward 8.3e-2 off
# RNE(ref) with +0.073 ulp of bias, bf16 dx 2.8e-3.  tests/test_groupnorm_numerics_cpu.py pins the cause; tests/test_gpu_groupnorm_rounding.py
# holds every GroupNorm route.


def _gn_stat_errors(x, B, G, L):
    """Error bounds of the 16-bit engines' GroupNorm statistics, derived from their arithmetic (norm.hip: sum and sum of squares in fp32 over
    at most 96 elements per thread, fp64 across threads, var = E[x^2] - mean^2 in fp64): per (sample, group) the relative error of rstd
    (<= 0.5 gamma_96 (mean^2 + var) / var + 8 u) and the absolute error of the mean (<= gamma_96 mean|x|).  The 1 + mean^2 / var factor is the
    amplification the kernel's comment calls harmless for means within tens of standard deviations: the 30 x std cases test that claim."""
    xg = x.reshape(B, G, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    er = 0.5 * N.gamma(96) * (mean ** 2 + var) / var + 8 * N.U32
    em = N.gamma(96) * xg.abs().mean(-1)
    return mean, var, er, em


@pytest.mark.parametrize("case", GN_CASES)
def test_groupnorm_against_float64(case):
    """GroupNorm (+ SiLU) forward and backward.  Intermediate rounding points read from norm.hip: none in the forward (z = xhat gamma + beta and
    SiLU in fp32, ONE rounding at the store), none before the dx store in the backward; the statistics carry the fp32-partial error bounded in
    _gn_stat_errors (an envelope of the arithmetic before the pivot; the per-route bounds are in test_gpu_groupnorm_rounding.py).  Forward: check A with d = 1.1 (|gamma| (|xhat| e_rstd + rstd e_mean) + 4 u |z|) + 8 u |y| (SiLU slope <= 1.1, __expf),
    plus check B.  Backward: dbeta (a plain column sum) check A; dgamma = sum dy xhat check A with the statistics' error added; dx check B."""
    G_ = _G(); c = G_.ctx()
    B, L, C, Gr, silu, off = case
    for dt in (1, 2):
        fmt = FMT[dt]
        x = N.to_storage(_randn((B, C, L), 71) + off, fmt)
        ga = N.rne(1 + 0.1 * _randn((C,), 72), "f32"); be = N.rne(0.1 * _randn((C,), 73), "f32")
        fwd = lambda x, ga, be: (F_silu(torch.nn.functional.group_norm(x, Gr, ga, be, eps=1e-6)) if silu else
                                 torch.nn.functional.group_norm(x, Gr, ga, be, eps=1e-6))
        ref = fwd(x, ga, be); emul = fwd(x.float(), ga.float(), be.float())
        mean, var, er, em = _gn_stat_errors(x, B, Gr, L)
        rstd = 1 / torch.sqrt(var + 1e-6)
        rep = lambda t: t.repeat_interleave(C // Gr, dim=1)[:, :, None]
        xhat = (x - rep(mean)) * rep(rstd)
        z = xhat * ga[:, None] + be[:, None]
        d = ga.abs()[:, None] * (xhat.abs() * rep(er) + rep(rstd) * rep(em)) + 4 * N.U32 * z.abs()
        if silu:
            d = 1.1 * d + 8 * N.U32 * ref.abs()
        xd = G_.nlc(x, dt); gad, bed = ga.float().to(G_.DEV), be.float().to(G_.DEV)
        yd = torch.empty(B * L, C, device=G_.DEV, dtype=G_.TDT[dt]); st = torch.empty(B * Gr * 2, device=G_.DEV)
        G_.check(G_.lib.eegldm_groupnorm_fwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(yd), C, G_.ptr(st), B, L, C, Gr, 1e-6, silu, 0,
                                             None, 0, dt))
        got = G_.ncl(yd, B, L).double()
        route = f"groupnorm fwd B{B} L{L} C{C} G{Gr} silu{silu} mean {off:g} std"
        # check A with the derived d: `check` takes d as gamma(n) * mag, so pass mag = d / gamma(0)
        N.check(got, ref, d / N.gamma(0), 0, fmt, route=route + " (check A)", min_stat=math.inf)     # (check B on the next line)
        N.check_b(got, ref, emul, fmt, route=route + " (check B)")
        # backward (the SiLU-free cases keep dgamma's bound exact: with SiLU its derivative at the perturbed z would enter too)
        dy = N.to_storage(_randn((B, C, L), 74), fmt)
        xr = x.clone().requires_grad_(True); gr = ga.clone().requires_grad_(True); br = be.clone().requires_grad_(True)
        (fwd(xr, gr, br) * dy).sum().backward()
        dyd = G_.nlc(dy, dt)
        dxd = torch.empty(B * L, C, device=G_.DEV, dtype=G_.TDT[dt]); dga = torch.zeros(C, device=G_.DEV); dbe = torch.zeros(C, device=G_.DEV)
        G_.check(G_.lib.eegldm_groupnorm_bwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(st), G_.ptr(dyd), C, G_.ptr(dxd), C,
                                             G_.ptr(dga), G_.ptr(dbe), B, L, C, Gr, silu, 0, None, 0, dt))
        torch.cuda.synchronize()
        x32 = x.float().requires_grad_(True)
        (fwd(x32, ga.float(), be.float()) * dy.float()).sum().backward()
        N.check_b(G_.ncl(dxd, B, L), xr.grad, x32.grad, fmt, route=route.replace("fwd", "bwd") + " dx")
        if not silu:
            N.check(dbe.cpu(), br.grad, dy.abs().sum((0, 2)), B * L, "f32", route=route.replace("fwd", "bwd") + " dbeta")
            dgd = N.gamma(B * L) * (dy * xhat).abs().sum((0, 2)) + (dy.abs() * (xhat.abs() * rep(er) + rep(rstd) * rep(em))).sum((0, 2))
            N.check(dga.cpu(), gr.grad, dgd / N.gamma(0), 0, "f32", route=route.replace("fwd", "bwd") + " dgamma")


def F_silu(t):
    return torch.nn.functional.silu(t)


# ---------------------------------------------------------------------------------------------------------------- non-finite dy through the other backward kernels
def _nonfinite_masks_agree(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    bad = (~torch.isfinite(got)) != (~torch.isfinite(ref))
    assert not bool(bad.any()), f"{what}: non-finite pattern differs in {int(bad.sum())} of {ref.numel()} elements " \
                                f"(kernel {int((~torch.isfinite(got)).sum())}, reference {int((~torch.isfinite(ref)).sum())} non-finite)"
    assert bool((~torch.isfinite(ref)).any()), what
    print(f"[nonfinite] {what}: {int((~torch.isfinite(ref)).sum())} non-finite elements, same pattern as the reference")


@pytest.mark.parametrize("dt", [1, 2])
def test_nonfinite_dy_through_groupnorm_attention_batchnorm(dt):
    """One NaN and one inf placed in dy must reach exactly the dx (and dgamma / dbeta) elements they reach in the float64 reference."""
    G_ = _G(); c = G_.ctx()
    fmt = FMT[dt]; td = G_.TDT[dt]
    # GroupNorm + SiLU
    B, L, C, Gr = 4, 192, 64, 32
    x = N.to_storage(_randn((B, C, L), 81), fmt); ga = N.rne(1 + 0.1 * _randn((C,), 82), "f32"); be = N.rne(0.1 * _randn((C,), 83), "f32")
    dy = _poison(N.to_storage(_randn((B, C, L), 84), fmt), [((1, 5, 17), math.nan), ((3, 40, 0), math.inf)])
    xr = x.clone().requires_grad_(True); gr = ga.clone().requires_grad_(True); br = be.clone().requires_grad_(True)
    (F_silu(torch.nn.functional.group_norm(xr, Gr, gr, br, eps=1e-6)) * dy).sum().backward()
    xd = G_.nlc(x, dt); gad, bed = ga.float().to(G_.DEV), be.float().to(G_.DEV)
    yd = torch.empty(B * L, C, device=G_.DEV, dtype=td); st = torch.empty(B * Gr * 2, device=G_.DEV)
    G_.check(G_.lib.eegldm_groupnorm_fwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(yd), C, G_.ptr(st), B, L, C, Gr, 1e-6, 1, 0, None, 0, dt))
    dyd = G_.nlc(dy, dt); dxd = torch.empty(B * L, C, device=G_.DEV, dtype=td); dga = torch.zeros(C, device=G_.DEV); dbe = torch.zeros(C, device=G_.DEV)
    G_.check(G_.lib.eegldm_groupnorm_bwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(st), G_.ptr(dyd), C, G_.ptr(dxd), C,
                                         G_.ptr(dga), G_.ptr(dbe), B, L, C, Gr, 1, 0, None, 0, dt))
    torch.cuda.synchronize()
    _nonfinite_masks_agree(G_.ncl(dxd, B, L), xr.grad, f"groupnorm bwd dx [{fmt}]")
    _nonfinite_masks_agree(dga, gr.grad, f"groupnorm bwd dgamma [{fmt}]")
    _nonfinite_masks_agree(dbe, br.grad, f"groupnorm bwd dbeta [{fmt}]")
    # attention (QKVAttentionLegacy, one head)
    from oracle.unet import qkv_attention
    B, T, Cc = 2, 64, 64
    qkv = N.to_storage(_randn((B, 3 * Cc, T), 85), fmt)
    do = _poison(N.to_storage(_randn((B, Cc, T), 86), fmt), [((0, 3, 10), math.nan), ((1, 60, 63), -math.inf)])
    qr = qkv.clone().requires_grad_(True)
    (qkv_attention(qr) * do).sum().backward()
    qd = G_.nlc(qkv, dt)
    od = torch.empty(B * T, Cc, device=G_.DEV, dtype=td); pr = torch.empty(B * T * T, device=G_.DEV, dtype=td)
    s1 = torch.empty(B * T * T, device=G_.DEV); s2 = torch.empty(B * T * T, device=G_.DEV, dtype=td)
    G_.check(G_.lib.eegldm_attention_fwd(c.h, G_.ptr(qd), 3 * Cc, G_.ptr(od), Cc, G_.ptr(pr), G_.ptr(s1), B, T, Cc, dt))
    dod = G_.nlc(do, dt); dq = torch.empty(B * T, 3 * Cc, device=G_.DEV, dtype=td)
    G_.check(G_.lib.eegldm_attention_bwd(c.h, G_.ptr(qd), 3 * Cc, G_.ptr(pr), G_.ptr(dod), Cc, G_.ptr(dq), 3 * Cc, G_.ptr(s1), G_.ptr(s2), B, T, Cc, dt))
    torch.cuda.synchronize()
    _nonfinite_masks_agree(G_.ncl(dq, B, T), qr.grad, f"attention bwd dqkv [{fmt}]")
    # BatchNorm (training statistics) + LeakyReLU(0.2)
    rows, C = 512, 64
    x = N.to_storage(_randn((rows, C), 87), fmt); ga = N.rne(1 + 0.1 * _randn((C,), 88), "f32"); be = N.rne(0.1 * _randn((C,), 89), "f32")
    dy = _poison(N.to_storage(_randn((rows, C), 90), fmt), [((100, 7), math.nan), ((3, 50), math.inf)])
    xr = x.clone().requires_grad_(True); gr = ga.clone().requires_grad_(True); br = be.clone().requires_grad_(True)
    mu_, var_ = xr.mean(0), xr.var(0, unbiased=False)
    (torch.nn.functional.leaky_relu((xr - mu_) / torch.sqrt(var_ + 1e-5) * gr + br, 0.2) * dy).sum().backward()
    xd = x.to(G_.DEV).to(td); gad, bed = ga.float().to(G_.DEV), be.float().to(G_.DEV)
    st = torch.zeros(4 * C, device=G_.DEV); rm = torch.zeros(C, device=G_.DEV); rv = torch.ones(C, device=G_.DEV); nbt = torch.zeros(1, device=G_.DEV)
    yd = torch.empty(rows, C, device=G_.DEV, dtype=td)
    G_.check(G_.lib.eegldm_batchnorm_lrelu_fwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(st), G_.ptr(rm), G_.ptr(rv), G_.ptr(nbt),
                                               G_.ptr(yd), C, rows, C, 0.2, 1, dt))
    dyd = dy.to(G_.DEV).to(td); dxd = torch.empty(rows, C, device=G_.DEV, dtype=td); dga = torch.zeros(C, device=G_.DEV); dbe = torch.zeros(C, device=G_.DEV)
    G_.check(G_.lib.eegldm_batchnorm_lrelu_bwd(c.h, G_.ptr(xd), C, G_.ptr(gad), G_.ptr(bed), G_.ptr(st), G_.ptr(dyd), C, G_.ptr(dxd), C,
                                               G_.ptr(dga), G_.ptr(dbe), rows, C, 0.2, dt))
    torch.cuda.synchronize()
    _nonfinite_masks_agree(dxd, xr.grad, f"batchnorm+lrelu bwd dx [{fmt}]")
    _nonfinite_masks_agree(dga, gr.grad, f"batchnorm+lrelu bwd dgamma [{fmt}]")
    _nonfinite_masks_agree(dbe, br.grad, f"batchnorm+lrelu bwd dbeta [{fmt}]")
