"""-m gpu: the thin-channel direct convolutions (csrc/direct_conv.hip), kernel by kernel, against correctly rounded float64 references
(tests/numerics.py, used unchanged: to_storage, evaluate, check A and B).

Every case names the kernel family that must serve it -- and the template channel counts where it has any -- and confirms it from
eegldm_debug_dconv_last_route; a case served by another kernel fails by name.  G = 4 channels per 16-byte group for f32 and 8 for the
16-bit types, so one shape may name different families per dtype: the tables say which.  Operands are float64 values already rounded to
the storage type, weights scaled 1 / sqrt(Cin K); every output buffer starts as NaN; with a leading dimension above the channel count the
gutter columns of the operands hold NaN (a kernel that reads them fails check A) and those of the output must still hold their NaN bit for
bit.  Reduction lengths: K Cin forward, K Cout data gradient, B Lout weight and bias gradient.  No tolerance is fitted.

Shapes are (B, L, Cin, Cout, K, stride, pad_l, pad_r).  What the entry points refuse is pinned as a refusal (non-zero return, message,
output untouched) instead of being run:
  eegldm_conv1d_fwd takes K in {1, 3} and stride in {1, 2} only, so the K = 2, K = 4, K = 5 and stride-3 FORWARD cases are refusals; the same
  kernels take those K through eegldm_conv1d_bwd_data, which has no such check: the K = 2 row / in1_seg cases, K = 4 thin_out and K = 5 point
  cases run as data gradients (of the mirrored conv where the family needs the other side wide).  thin_out_run has no data-gradient mode,
  so its K = 2 cases exist only as the refusal.  The stride-3 in1_seg case cannot "fall to thin_in_reg": forward refuses it, and as a data
  gradient it has a wide input side.
  (2,40,12,12,3,1,1,1) counts as thin (a side under 16) but has no side <= 8: forward and bwd_data refuse before any launch, bwd_weight
  runs the generic kernel.
  (2,64,32,24,3,1,1,1) is NOT thin in any dtype (both sides >= 16 and multiples of 8): its weight gradient is asserted to run on the MFMA
  GEMM; (2,64,32,20,...) takes its place as the wide generic case of the 16-bit types.
Wrap cases (grid-stride loop taken more than once; N = CU count, the forward grid cap is 16 N blocks): one per family that has such a
loop, one dtype each; in1_seg and in1out size their grid to the problem and have none.  The thin_out_run wrap needs 3.4e7 operand elements
(f32, the only type under 4e7) and is the largest case of the file.

Coverage, family x mode x dtype (every entry asserted from the route record; "all" = f32, bf16, f16):
  row           forward all (16 <CI,CO> + padded 3->5, 7->6, K1, stride 2, scalar ld path, wrap bf16); data gradient all (K2 both pads, odd L)
  in1_seg       forward all (Lo 64, 129, stride 2, pads (0,2) (2,0), K1; Cout 512 16-bit); data gradient all (K1, K2, Lout != L)
  thin_in_reg   forward all (CI 1, 2, 4; stride 2; K1; wrap bf16); data gradient all (CI 1, 2, 4)
  thin_in       forward all (6->32, 8->16 stride 2, 3->24; f32 2->20; wrap bf16); data gradient all (32->6; f32 20->2)
  thin_out_run  forward all (32->1, one run per sample, 16->1, 256->1, pads, K1; 512->1 16-bit; wrap f32); no data-gradient mode
  thin_out      forward all (32->3, 64->8 stride 2, Lo 60; 512->2 16-bit; wrap f32); data gradient all (stride 2, K4, K5)
  rowdot        forward all (24->2, 100->3; f32 512->1, 512->2; wrap bf16); data gradient all
  point         forward all (2->18, ldout 33; 16-bit 2->20; wrap bf16); data gradient all (K5 32->2, 3->3; 16-bit 20->2)
  tinyv         all (9 <CI,CO>, stride 2, K1, K2, 65 blocks, bias fused / by colsum, wrap bf16, deterministic)
  tiny          all (3->3, 3->1, ldx 3; wrap bf16; deterministic)
  in1out        bf16, the only type it serves (3 / 24 / 16 segments, pads, K2, L 1025 -> wt; deterministic)
  wt            wide Cout all, wide Cin all (32->1: f32, f16); wrap bf16 (wide Cout); deterministic both
  generic       all (K5 2->2, 12->12; 16-bit 32->20; wrap bf16; deterministic)
16-bit forward and data-gradient families each have one shape of >= 131072 outputs for check B; non-finite operands: one case or more per
family and mode; fp16 range: row, in1_seg, thin_out_run; fused LeakyReLU: in1_seg and thin_in_reg, f32 and bf16.

Each check prints one `[numerics]` line (route, element count, reduction length, worst error over bound, and for 16-bit outputs the
mismatch share against the emulation's and the mean signed ulp), each launch one `[route]` line."""
import ctypes
import csv
import math
import os
import tempfile

import numpy as np
import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

FMT = {0: "f32", 1: "bf16", 2: "f16"}
ALL, H = (0, 1, 2), (1, 2)
ROW, SEG, REG, LDS, RUN, OUT, DOT, PT = 1, 2, 3, 4, 5, 6, 7, 8
FWD_NAME = {0: "none", ROW: "row", SEG: "in1_seg", REG: "thin_in_reg", LDS: "thin_in", RUN: "thin_out_run", OUT: "thin_out", DOT: "rowdot", PT: "point"}
TINYV, TINY, IN1OUT, WT, GEN = 1, 2, 3, 4, 5
WG_NAME = {0: "none", TINYV: "tinyv", TINY: "tiny", IN1OUT: "in1out", WT: "wt", GEN: "generic"}
GEMM = "gemm"           # a case that must NOT be served by the direct kernels


def _G():
    import gpu_util as G
    return G


def _randn(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _lout(L, K, s, pl, pr):
    return (L + pl + pr - K) // s + 1


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _route(G, which):
    out = (ctypes.c_int * 8)()
    G.check(G.lib.eegldm_debug_dconv_last_route(which, out))
    return dict(family=out[0], ci=out[1], co=out[2], dgrad=out[3], blocks=out[4], rpb=out[5], parts=out[6], det=out[7])


def _want(spec, dt):
    """spec: family | (family, ci) | (family, ci, co), or a dict of those per dtype"""
    if isinstance(spec, dict):
        spec = spec[dt]
    if not isinstance(spec, tuple):
        spec = (spec,)
    return spec + (None,) * (3 - len(spec))


def _confirm(G, which, spec, dt, tag, dgrad=None):
    fam, ci, co = _want(spec, dt)
    got = _route(G, which)
    names = WG_NAME if which else FWD_NAME
    assert got["family"] == fam, f"{tag}: served by {names.get(got['family'], got['family'])} {got}, expected {names[fam]}"
    if ci is not None:
        assert got["ci"] == ci, f"{tag}: template CI = {got['ci']}, expected {ci} ({got})"
    if co is not None:
        assert got["co"] == co, f"{tag}: template CO = {got['co']}, expected {co} ({got})"
    if dgrad is not None:
        assert got["dgrad"] == dgrad, f"{tag}: dgrad flag {got['dgrad']}, expected {dgrad}"
    print(f"[route] {tag}: {names[fam]} CI={got['ci']} CO={got['co']} dgrad={got['dgrad']} blocks={got['blocks']} rows/block={got['rpb']} "
          f"parts={got['parts']} det={got['det']}")
    return got


def _dev(t_ncl, G, dt, ld=None):
    """(B, C, L) float64 -> device NLC [(B L), ld]; gutter columns hold NaN"""
    B, C, L = t_ncl.shape
    t = t_ncl.permute(0, 2, 1).reshape(B * L, C).to(G.TDT[dt])
    if ld is None or ld == C:
        return t.contiguous().to(G.DEV)
    buf = torch.full((B * L, ld), float("nan"), dtype=G.TDT[dt])
    buf[:, :C] = t
    return buf.to(G.DEV)


def _out_buf(G, dt, rows, C, ld=None):
    return torch.full((rows, ld or C), float("nan"), device=G.DEV, dtype=G.TDT[dt])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _gutter_untouched(buf, C, before_bits, tag):
    if buf.shape[1] > C:
        assert torch.equal(_bits(buf[:, C:].contiguous()), before_bits), f"{tag}: gutter columns of the output were written"


def _poison3(t, edge=0):
    """+inf at position `edge` of sample 0 (last channel), -inf at position L - 1 - edge of the last sample (channel 0), NaN mid-sample.
    edge = 0 everywhere but in the dy of a weight gradient: there a boundary row of dy meets a ZERO of the padding in the reference
    (numerics.conv1d_wgrad pads x with F.pad, and inf * 0 = NaN), a product no kernel forms and the existing suite avoids the same way
    (test_gpu_rounding._wgrad_case poisons row 1); rows 1 and L - 2 of a K = 3, pad 1, stride 1 conv touch no padding."""
    t = t.clone()
    B, C, L = t.shape
    t[0, C - 1, edge] = math.inf
    t[B - 1, 0, L - 1 - edge] = -math.inf
    t[B - 1, 1 % C, L // 2] = math.nan
    return t


def _nonfinite_same(got, ref, tag):
    got, ref = N._f64(got), N._f64(ref)
    nr = ~torch.isfinite(ref)
    assert bool(nr.any()), f"{tag}: the reference has no non-finite element"
    bad = nr != ~torch.isfinite(got)
    assert not bool(bad.any()), (f"{tag}: non-finite pattern differs in {int(bad.sum())} of {ref.numel()} elements "
                                 f"(kernel {int((~torch.isfinite(got)).sum())}, reference {int(nr.sum())} non-finite)")
    inf_r = torch.isinf(ref)
    assert bool((got[inf_r] == ref[inf_r]).all()), f"{tag}: an infinite reference element is not the same infinity in the output"
    print(f"[nonfinite] {tag}: {int(nr.sum())} non-finite elements ({int(inf_r.sum())} inf), same pattern as the reference")


# ---------------------------------------------------------------------------------------------------------------- runners
def _fwd(G, c, name, shape, dt, spec, ep="", ld=None, scale=1.0, poison=False, tag="", wrap=False):
    B, L, Cin, Cout, K, s, pl, pr = shape
    fmt = FMT[dt]
    Lout = _lout(L, K, s, pl, pr)
    ldin, ldout, ldr = ld or (Cin, Cout, Cout)
    x = N.to_storage(_randn((B, Cin, L), 1), fmt)
    w = N.to_storage(_randn((Cout, Cin, K), 2, scale / math.sqrt(Cin * K)), fmt)
    assert bool(torch.isfinite(w).all()), f"{name}: a weight overflows {fmt} at scale {scale}"
    if poison:
        x = _poison3(x)
    b = N.rne(_randn((Cout,), 3, scale), "f32") if "b" in ep else None
    res = N.to_storage(_randn((B, Cout, Lout), 5, scale), fmt) if "s" in ep else None
    ref, mag, emul = N.evaluate(N.conv1d_fwd, x, w, b, s, pl, pr, None, res)
    if fmt == "f16" and scale > 1:          # the range cases must reach their range, asserted from the reference alone
        assert float(torch.isinf(N.rne(ref, "f16")).double().mean()) > 1e-3, f"{name}: no output overflows fp16 at scale {scale}"
    if fmt == "f16" and scale < 1:
        r16 = N.rne(ref, "f16")
        assert float(((r16 != 0) & (r16.abs() < 2.0 ** -14)).double().mean()) > 0.5, f"{name}: outputs not in the fp16 subnormal range"
    xd, wd = _dev(x, G, dt, ldin), G.pack_w(w, dt)
    bd = b.float().to(G.DEV) if b is not None else None
    sd = _dev(res, G, dt, ldr) if res is not None else None
    yd = _out_buf(G, dt, B * Lout, Cout, ldout)
    gut = _bits(yd[:, Cout:].contiguous()) if ldout > Cout else None
    G.check(G.lib.eegldm_conv1d_fwd(c.h, G.ptr(xd), ldin, G.ptr(wd), G.ptr(bd), G.ptr(yd), ldout, B, L, Cin, Cout, K, s, pl, pr,
                                    None, 0, G.ptr(sd), ldr if sd is not None else 0, dt))
    torch.cuda.synchronize()
    route = f"thin fwd {name} [{ep or '-'}]{tag}"
    got = _confirm(G, 0, spec, dt, route + " " + fmt, dgrad=0)
    if wrap:
        assert got["blocks"] * got["rpb"] < B * Lout, f"{route}: the grid-stride loop did not wrap ({got}, rows {B * Lout})"
    _gutter_untouched(yd, Cout, gut, route)
    y = G.ncl(yd[:, :Cout].contiguous(), B, Lout)
    if poison:
        _nonfinite_same(y, ref, route + " " + fmt)
    if fmt == "f16" and scale < 1:           # subnormal outputs must EQUAL RNE(ref) wherever the bound leaves one candidate
        d = N.gamma(K * Cin) * mag
        r16 = N.rne(ref, "f16")
        one = (r16 != 0) & (r16.abs() < 2.0 ** -14) & (N.rne(ref - d, "f16") == N.rne(ref + d, "f16"))
        assert bool((y.double()[one] == r16[one]).all()), f"{route}: fp16-subnormal outputs differ from RNE(ref)"
    return N.check(y, ref, mag, K * Cin, fmt, emul=emul, route=route)


def _dgrad(G, c, name, shape, dt, spec, rs=False, ld=None, poison=False, tag="", wrap=False):
    B, L, Cin, Cout, K, s, pl, pr = shape
    fmt = FMT[dt]
    Lout = _lout(L, K, s, pl, pr)
    lddy, lddx, ldr = ld or (Cout, Cin, Cin)
    w = N.to_storage(_randn((Cout, Cin, K), 21, 1 / math.sqrt(Cout * K)), fmt)
    dy = N.to_storage(_randn((B, Cout, Lout), 22), fmt)
    if poison:
        dy = _poison3(dy)
    res = N.to_storage(_randn((B, Cin, L), 23), fmt) if rs else None
    ref, mag, emul = N.evaluate(N.conv1d_dgrad, dy, w, L, s, pl, pr, res)
    dyd, wd = _dev(dy, G, dt, lddy), G.pack_w(w, dt)
    rd = _dev(res, G, dt, ldr) if rs else None
    dxd = _out_buf(G, dt, B * L, Cin, lddx)
    gut = _bits(dxd[:, Cin:].contiguous()) if lddx > Cin else None
    G.check(G.lib.eegldm_conv1d_bwd_data(c.h, G.ptr(dyd), lddy, G.ptr(wd), G.ptr(dxd), lddx, B, L, Cin, Cout, K, s, pl, pr,
                                         G.ptr(rd), ldr if rs else 0, dt))
    torch.cuda.synchronize()
    route = f"thin dgrad {name} [{'+resid' if rs else '-'}]{tag}"
    got = _confirm(G, 0, spec, dt, route + " " + fmt, dgrad=1)
    if wrap:
        assert got["blocks"] * got["rpb"] < B * L, f"{route}: the grid-stride loop did not wrap ({got}, rows {B * L})"
    _gutter_untouched(dxd, Cin, gut, route)
    dx = G.ncl(dxd[:, :Cin].contiguous(), B, L)
    if poison:
        _nonfinite_same(dx, ref, route + " " + fmt)
    return N.check(dx, ref, mag, K * Cout, fmt, emul=emul, route=route)


def _prof_rows(G, c):
    path = os.path.join(tempfile.gettempdir(), f"eegldm_thin_rows_{os.getpid()}.csv")
    G.check(G.lib.eegldm_prof_dump(c.h, path.encode()))
    with open(path) as fh:
        return list(csv.DictReader(fh))


def _wgrad(G, c, name, shape, dt, spec, accumulate=False, poison=None, ldx=None, tag="", wrap=False, det=None, keep_from=None):
    B, L, Cin, Cout, K, s, pl, pr = shape
    fmt = FMT[dt]
    Lout = _lout(L, K, s, pl, pr)
    x = N.to_storage(_randn((B, Cin, L), 31), fmt)
    dy = N.to_storage(_randn((B, Cout, Lout), 32), fmt)
    if poison == "x":
        x = _poison3(x)
    if poison == "dy":
        assert (K, s, pl, pr) == (3, 1, 1, 1)
        dy = _poison3(dy, edge=1)
    if keep_from is not None:               # zero every dy row the first grid-stride pass owns: dW and db are sums over the wrapped rows alone
        flat = dy.permute(0, 2, 1).reshape(B * Lout, Cout).clone()
        flat[:keep_from] = 0
        dy = flat.reshape(B, Lout, Cout).permute(0, 2, 1).contiguous()
    acc_w = N.rne(_randn((Cout, Cin, K), 33, 8.0), "f32") if accumulate else None
    acc_b = N.rne(_randn((Cout,), 34, 8.0), "f32") if accumulate else None
    ref, mag, _ = N.evaluate(N.conv1d_wgrad, x, dy, K, s, pl, pr, acc_w)
    bref, bmag, _ = N.evaluate(N.bias_grad, dy, acc_b)
    xd, dyd = _dev(x, G, dt, ldx), _dev(dy, G, dt)
    dwd = G.pack_w(acc_w.float(), 0) if accumulate else torch.zeros(K, Cout, Cin, device=G.DEV)
    dbd = acc_b.float().to(G.DEV) if accumulate else torch.zeros(Cout, device=G.DEV)
    route = f"thin wgrad {name}{tag}" + (" [+= non-zero]" if accumulate else "") + (f" [NaN/inf in {poison}]" if poison else "")
    if spec == GEMM:
        c.prof_enable(True)
    try:
        G.check(G.lib.eegldm_conv1d_bwd_weight(c.h, G.ptr(xd), ldx or Cin, G.ptr(dyd), Cout, G.ptr(dwd), G.ptr(dbd), B, L, Cin, Cout, K, s, pl, pr, dt))
        torch.cuda.synchronize()
        if spec == GEMM:
            rows = _prof_rows(G, c)
            assert rows, f"{route}: expected the MFMA GEMM family, the profiler saw no launch"
            print(f"[route] {route} {fmt}: {rows[0]['kernel']} (not a thin conv)")
    finally:
        if spec == GEMM:
            c.prof_enable(False)
    if spec != GEMM:
        got = _confirm(G, 1, spec, dt, route + " " + fmt)
        if det is not None:
            assert got["det"] == det, f"{route}: deterministic flag {got['det']}"
        if wrap:
            assert got["blocks"] * got["rpb"] < B * Lout, f"{route}: the grid-stride loop did not wrap ({got}, rows {B * Lout})"
    n = B * Lout
    dw = G.unpack_w(dwd)
    if poison:
        _nonfinite_same(dw, ref, route + " dW " + fmt)
    N.check(dw, ref, mag, n, "f32", route=route + f" dW [{fmt} operands]")
    N.check(dbd.cpu(), bref, bmag, n, "f32", route=route + f" db [{fmt} operands]")
    return dwd, dbd


# ---------------------------------------------------------------------------------------------------------------- forward
# name, shape, dtypes, expected family (per dtype where it differs), leading dimensions (ldin, ldout, ld_resid) or None
def _row_grid():
    return [(f"row {ci}->{co}", (2, 19, ci, co, 3, 1, 1, 1), ALL, (ROW, ci, co), None) for ci in (1, 2, 4, 8) for co in (1, 2, 4, 8)]


FWD_CASES = _row_grid() + [
    ("row 1->1 three samples", (3, 37, 1, 1, 3, 1, 1, 1), ALL, (ROW, 1, 1), None),
    ("row 2->4 stride 2", (2, 50, 2, 4, 3, 2, 1, 1), ALL, (ROW, 2, 4), None),
    ("row padded 3->5", (2, 33, 3, 5, 3, 1, 1, 1), ALL, (ROW, 4, 8), None),
    ("row padded 7->6", (2, 33, 7, 6, 3, 1, 1, 1), ALL, (ROW, 8, 8), None),
    ("row K1 4->8", (2, 40, 4, 8, 1, 1, 0, 0), ALL, (ROW, 4, 8), None),
    ("row 4->4 ldin 5 ldout 7 ld_resid 5 (scalar in / out)", (2, 19, 4, 4, 3, 1, 1, 1), ALL, (ROW, 4, 4), (5, 7, 5)),
    ("in1_seg Lo 64 (smallest accepted)", (2, 64, 1, 16, 3, 1, 1, 1), ALL, SEG, None),
    ("in1_seg Lo 63 -> thin_in_reg", (2, 63, 1, 16, 3, 1, 1, 1), ALL, (REG, 1), None),
    ("in1_seg one row in the last segment", (3, 129, 1, 32, 3, 1, 1, 1), ALL, SEG, None),
    ("in1_seg stride 2 segments 128 + 22", (2, 300, 1, 64, 3, 2, 1, 1), ALL, SEG, None),
    ("in1_seg pads (0,2)", (2, 130, 1, 16, 3, 1, 0, 2), ALL, SEG, None),
    ("in1_seg pads (2,0)", (2, 130, 1, 16, 3, 1, 2, 0), ALL, SEG, None),
    ("in1_seg K1", (2, 130, 1, 16, 1, 1, 0, 0), ALL, SEG, None),
    ("in1_seg Cout 512 (64 groups, 4 rows per block pass)", (2, 130, 1, 512, 3, 1, 1, 1), H, SEG, None),
    ("thin_in_reg 2->32", (2, 64, 2, 32, 3, 1, 1, 1), ALL, (REG, 2), None),
    ("thin_in_reg 4->64 stride 2", (2, 64, 4, 64, 3, 2, 1, 1), ALL, (REG, 4), None),
    ("thin_in_reg K1 2->16", (2, 40, 2, 16, 1, 1, 0, 0), ALL, (REG, 2), None),
    ("thin_in 6->32", (2, 64, 6, 32, 3, 1, 1, 1), ALL, LDS, None),
    ("thin_in 8->16 stride 2", (2, 64, 8, 16, 3, 2, 1, 1), ALL, LDS, None),
    ("thin_in 3->24 (groups do not divide 256)", (2, 64, 3, 24, 3, 1, 1, 1), ALL, LDS, None),
    ("thin_out_run 32->1", (2, 64, 32, 1, 3, 1, 1, 1), ALL, RUN, None),
    ("thin_out_run one run per sample", (3, 8, 32, 1, 3, 1, 1, 1), ALL, RUN, None),
    ("thin_out_run 512->1 (16-bit: 64-lane butterfly; f32: 128 groups -> rowdot)", (2, 24, 512, 1, 3, 1, 1, 1), ALL, {0: DOT, 1: RUN, 2: RUN}, None),
    ("thin_out_run 256->1 (f32: 64-lane butterfly)", (2, 24, 256, 1, 3, 1, 1, 1), ALL, RUN, None),
    ("thin_out_run 16->1", (2, 16, 16, 1, 3, 1, 1, 1), ALL, RUN, None),
    ("thin_out_run pads (0,2)", (2, 64, 32, 1, 3, 1, 0, 2), ALL, RUN, None),
    ("thin_out_run pads (2,0)", (2, 64, 32, 1, 3, 1, 2, 0), ALL, RUN, None),
    ("thin_out_run K1", (2, 64, 32, 1, 1, 1, 0, 0), ALL, RUN, None),
    ("thin_out_run Lo 60 -> thin_out", (2, 60, 32, 1, 3, 1, 1, 1), ALL, OUT, None),
    ("thin_out 32->3", (2, 64, 32, 3, 3, 1, 1, 1), ALL, OUT, None),
    ("thin_out 64->8 stride 2", (2, 60, 64, 8, 3, 2, 1, 1), ALL, OUT, None),
    ("thin_out 512->2 (f32: 128 groups -> rowdot)", (2, 20, 512, 2, 3, 1, 1, 1), ALL, {0: DOT, 1: OUT, 2: OUT}, None),
    ("rowdot 24->2 (groups not a power of two)", (2, 40, 24, 2, 3, 1, 1, 1), ALL, DOT, None),
    ("rowdot 100->3 (lane loop tail)", (2, 40, 100, 3, 3, 1, 1, 1), ALL, DOT, None),
    ("point 2->20 (f32: 5 groups -> thin_in)", (2, 40, 2, 20, 3, 1, 1, 1), ALL, {0: LDS, 1: PT, 2: PT}, None),
    ("point 2->18", (2, 40, 2, 18, 3, 1, 1, 1), ALL, PT, None),
    ("point 2->32 ldout 33", (2, 40, 2, 32, 3, 1, 1, 1), ALL, PT, (2, 33, 32)),
]


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_forward(case):
    G = _G(); c = G.ctx()
    name, shape, dts, spec, ld = case
    for dt in dts:
        for ep in ("", "b", "bs"):
            _fwd(G, c, name, shape, dt, spec, ep=ep, ld=ld)


# one wrap case per family with a grid-stride loop: shape as a function of the CU count, dtype, family
FWD_WRAP = [
    ("row", lambda n: (2, 8 * n * 256 + 77, 1, 1, 3, 1, 1, 1), 1, (ROW, 1, 1)),
    ("thin_in_reg", lambda n: (2, 8 * n * 4 + 50, 2, 512, 3, 1, 1, 1), 1, (REG, 2)),
    ("thin_in", lambda n: (2, 1024 * n + 40, 8, 16, 3, 1, 1, 1), 1, LDS),
    ("thin_out_run", lambda n: (2, 4096 * n + 8, 16, 1, 3, 1, 1, 1), 0, RUN),
    ("thin_out", lambda n: (2, 8 * n * 64 + 30, 16, 2, 3, 1, 1, 1), 0, OUT),
    ("rowdot", lambda n: (2, 32 * n + 10, 24, 2, 3, 1, 1, 1), 1, DOT),
    ("point", lambda n: (2, 8 * n * 13 + 5, 2, 20, 3, 1, 1, 1), 1, PT),          # 13 = ceil(256 / 20) rows per block pass
]


@pytest.mark.parametrize("case", FWD_WRAP, ids=[c[0] for c in FWD_WRAP])
def test_forward_grid_stride_wrap(case):
    G = _G(); c = G.ctx()
    name, shape_of, dt, spec = case
    _fwd(G, c, "wrap " + name, shape_of(_cus()), dt, spec, ep="b", wrap=True)


# check B: one shape of >= 131072 output elements per family with 16-bit outputs
FWD_BIG = [
    ("row", (4, 8192, 2, 4, 3, 1, 1, 1), (ROW, 2, 4)),
    ("in1_seg", (4, 512, 1, 64, 3, 1, 1, 1), SEG),
    ("thin_in_reg", (4, 512, 2, 64, 3, 1, 1, 1), (REG, 2)),
    ("thin_in", (4, 512, 6, 64, 3, 1, 1, 1), LDS),
    ("thin_out_run", (4, 32768, 32, 1, 3, 1, 1, 1), RUN),
    ("thin_out", (4, 4096, 32, 8, 3, 1, 1, 1), OUT),
    ("rowdot", (4, 4096, 24, 8, 3, 1, 1, 1), DOT),
    ("point", (4, 512, 2, 68, 3, 1, 1, 1), PT),
]


@pytest.mark.parametrize("case", FWD_BIG, ids=[c[0] for c in FWD_BIG])
def test_forward_check_b(case):
    G = _G(); c = G.ctx()
    name, shape, spec = case
    for dt in H:
        st = _fwd(G, c, "check B " + name, shape, dt, spec, ep="bs")
        assert st["n_elem"] >= 131072 and "m_emul" in st


# ---------------------------------------------------------------------------------------------------------------- refusals
REFUSED = [
    ("fwd K2 row pads (0,1)", "fwd", (2, 40, 8, 2, 2, 1, 0, 1), "unsupported conv"),
    ("fwd K2 row pads (1,0)", "fwd", (2, 40, 8, 2, 2, 1, 1, 0), "unsupported conv"),
    ("fwd K2 in1_seg", "fwd", (2, 130, 1, 16, 2, 1, 0, 1), "unsupported conv"),
    ("fwd K2 thin_out_run pads (0,1)", "fwd", (2, 64, 32, 1, 2, 1, 0, 1), "unsupported conv"),
    ("fwd K2 thin_out_run pads (1,0)", "fwd", (2, 64, 32, 1, 2, 1, 1, 0), "unsupported conv"),
    ("fwd K4 thin_out", "fwd", (2, 40, 8, 8, 4, 2, 1, 1), "unsupported conv"),
    ("fwd K5 point 2->32", "fwd", (2, 40, 2, 32, 5, 1, 2, 2), "unsupported conv"),
    ("fwd K5 point 3->3", "fwd", (2, 40, 3, 3, 5, 1, 2, 2), "unsupported conv"),
    ("fwd stride 3 in1_seg", "fwd", (2, 200, 1, 16, 3, 3, 1, 1), "unsupported conv"),
    ("fwd 12->12 no side <= 8", "fwd", (2, 40, 12, 12, 3, 1, 1, 1), "direct conv expects a thin side"),
    ("bwd_data 12->12 no side <= 8", "dgrad", (2, 40, 12, 12, 3, 1, 1, 1), "direct conv expects a thin side"),
]


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_refused_shapes_fail_loudly_before_any_launch(case):
    G = _G(); c = G.ctx()
    name, which, (B, L, Cin, Cout, K, s, pl, pr), msg = case
    Lout = _lout(L, K, s, pl, pr)
    for dt in ALL:
        fmt = FMT[dt]
        w = G.pack_w(N.to_storage(_randn((Cout, Cin, K), 2), fmt), dt)
        if which == "fwd":
            src = _dev(N.to_storage(_randn((B, Cin, L), 1), fmt), G, dt); dst = _out_buf(G, dt, B * Lout, Cout)
            before = _bits(dst).clone()
            rc = G.lib.eegldm_conv1d_fwd(c.h, G.ptr(src), Cin, G.ptr(w), None, G.ptr(dst), Cout, B, L, Cin, Cout, K, s, pl, pr, None, 0, None, 0, dt)
        else:
            src = _dev(N.to_storage(_randn((B, Cout, Lout), 1), fmt), G, dt); dst = _out_buf(G, dt, B * L, Cin)
            before = _bits(dst).clone()
            rc = G.lib.eegldm_conv1d_bwd_data(c.h, G.ptr(src), Cout, G.ptr(w), G.ptr(dst), Cin, B, L, Cin, Cout, K, s, pl, pr, None, 0, dt)
        torch.cuda.synchronize()
        err = G.lib.eegldm_last_error().decode(errors="replace")
        assert rc != 0, f"{name} [{fmt}]: accepted"
        assert msg in err, f"{name} [{fmt}]: message {err!r}"
        assert torch.equal(_bits(dst), before), f"{name} [{fmt}]: the output was written"
        print(f"[refused] {name} [{fmt}]: rc {rc}: {err}")


# ---------------------------------------------------------------------------------------------------------------- data gradient
# name, conv shape, dtypes, family reached (launch input side = Cout, output side = Cin), leading dimensions (lddy, lddx, ld_resid)
DGRAD_CASES = [
    ("row 2->2", (2, 19, 2, 2, 3, 1, 1, 1), ALL, (ROW, 2, 2), None),
    ("row 2->4", (2, 19, 2, 4, 3, 1, 1, 1), ALL, (ROW, 4, 2), None),
    ("row 4->2", (2, 19, 4, 2, 3, 1, 1, 1), ALL, (ROW, 2, 4), None),
    ("row 4->4", (2, 19, 4, 4, 3, 1, 1, 1), ALL, (ROW, 4, 4), None),
    ("row 2->4 stride 2", (2, 50, 2, 4, 3, 2, 1, 1), ALL, (ROW, 4, 2), None),
    ("row 2->4 stride 2 odd length", (2, 51, 2, 4, 3, 2, 1, 1), ALL, (ROW, 4, 2), None),
    ("row 4->4 lddy 5 lddx 7 ld_resid 5", (2, 19, 4, 4, 3, 1, 1, 1), ALL, (ROW, 4, 4), (5, 7, 5)),
    ("row K2 8->2 pads (0,1)", (2, 40, 8, 2, 2, 1, 0, 1), ALL, (ROW, 2, 8), None),
    ("row K2 8->2 pads (1,0)", (2, 40, 8, 2, 2, 1, 1, 0), ALL, (ROW, 2, 8), None),
    ("in1_seg 32->1", (2, 130, 32, 1, 3, 1, 1, 1), ALL, SEG, None),
    ("in1_seg 32->1 no padding (Lout != L)", (2, 130, 32, 1, 3, 1, 0, 0), ALL, SEG, None),
    ("in1_seg K2 16->1 pads (0,1)", (2, 130, 16, 1, 2, 1, 0, 1), ALL, SEG, None),
    ("in1_seg K2 16->1 pads (1,0)", (2, 130, 16, 1, 2, 1, 1, 0), ALL, SEG, None),
    ("in1_seg K1 16->1", (2, 130, 16, 1, 1, 1, 0, 0), ALL, SEG, None),
    ("in1_seg stride 2 16->1 -> thin_in_reg", (2, 130, 16, 1, 3, 2, 1, 1), ALL, (REG, 1), None),
    ("thin_in_reg 32->2", (2, 64, 32, 2, 3, 1, 1, 1), ALL, (REG, 2), None),
    ("thin_in_reg 32->4 stride 2", (2, 64, 32, 4, 3, 2, 1, 1), ALL, (REG, 4), None),
    ("thin_in 32->6", (2, 64, 32, 6, 3, 1, 1, 1), ALL, LDS, None),
    ("thin_out 4->64 stride 2", (2, 64, 4, 64, 3, 2, 1, 1), ALL, OUT, None),
    ("thin_out 3->32", (2, 64, 3, 32, 3, 1, 1, 1), ALL, OUT, None),
    ("thin_out K4 8->8 stride 2", (2, 40, 8, 8, 4, 2, 1, 1), ALL, OUT, None),
    ("thin_out K5 2->32", (2, 40, 2, 32, 5, 1, 2, 2), ALL, OUT, None),
    ("rowdot 2->24", (2, 40, 2, 24, 3, 1, 1, 1), ALL, DOT, None),
    ("rowdot 3->100", (2, 40, 3, 100, 3, 1, 1, 1), ALL, DOT, None),
    ("point 20->2 (f32: 5 groups -> thin_in)", (2, 40, 20, 2, 3, 1, 1, 1), ALL, {0: LDS, 1: PT, 2: PT}, None),
    ("point K5 32->2", (2, 40, 32, 2, 5, 1, 2, 2), ALL, PT, None),
    ("point K5 3->3", (2, 40, 3, 3, 5, 1, 2, 2), ALL, PT, None),
]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[c[0] for c in DGRAD_CASES])
def test_data_gradient(case):
    G = _G(); c = G.ctx()
    name, shape, dts, spec, ld = case
    for dt in dts:
        for rs in (False, True):
            _dgrad(G, c, name, shape, dt, spec, rs=rs, ld=ld)


DGRAD_BIG = [
    ("row", (4, 8192, 4, 2, 3, 1, 1, 1), (ROW, 2, 4)),
    ("in1_seg", (4, 512, 64, 1, 3, 1, 1, 1), SEG),
    ("thin_in_reg", (4, 512, 64, 2, 3, 1, 1, 1), (REG, 2)),
    ("thin_in", (4, 512, 64, 6, 3, 1, 1, 1), LDS),
    ("thin_out", (4, 4096, 8, 32, 3, 1, 1, 1), OUT),
    ("rowdot", (4, 4096, 8, 24, 3, 1, 1, 1), DOT),
    ("point", (4, 512, 68, 2, 3, 1, 1, 1), PT),
]


@pytest.mark.parametrize("case", DGRAD_BIG, ids=[c[0] for c in DGRAD_BIG])
def test_data_gradient_check_b(case):
    G = _G(); c = G.ctx()
    name, shape, spec = case
    for dt in H:
        st = _dgrad(G, c, "check B " + name, shape, dt, spec, rs=True)
        assert st["n_elem"] >= 131072 and "m_emul" in st


# ---------------------------------------------------------------------------------------------------------------- weight + bias gradient
# name, shape, dtypes, family (wt: CI = 1 wide Cout, 0 wide Cin), ldx or None
def _tinyv_grid():
    return [(f"tinyv {ci}->{co}", (2, 37, ci, co, 3, 1, 1, 1), ALL, (TINYV, ci, co), None) for ci in (1, 2, 4) for co in (1, 2, 4)]


WGRAD_CASES = _tinyv_grid() + [
    ("tinyv 2->4 stride 2", (2, 50, 2, 4, 3, 2, 1, 1), ALL, (TINYV, 2, 4), None),
    ("tinyv K1 2->4", (2, 37, 2, 4, 1, 1, 0, 0), ALL, (TINYV, 2, 4), None),
    ("tinyv K2 2->4", (2, 37, 2, 4, 2, 1, 0, 1), ALL, (TINYV, 2, 4), None),
    ("tinyv 65 blocks (the 8-block fold)", (2, 8200, 2, 4, 3, 1, 1, 1), ALL, (TINYV, 2, 4), None),
    ("tiny 3->3", (2, 37, 3, 3, 3, 1, 1, 1), ALL, TINY, None),
    ("tiny 3->1", (2, 37, 3, 1, 3, 1, 1, 1), ALL, TINY, None),
    ("tiny 2->4 ldx 3", (2, 37, 2, 4, 3, 1, 1, 1), ALL, TINY, 3),
    ("in1out 3 segments per sample", (2, 192, 32, 1, 3, 1, 1, 1), (1,), IN1OUT, None),
    ("in1out 512->1, 24 segments of 4 rows", (2, 96, 512, 1, 3, 1, 1, 1), (1,), IN1OUT, None),
    ("in1out L 1024 (largest accepted)", (2, 1024, 32, 1, 3, 1, 1, 1), (1,), IN1OUT, None),
    ("in1out L 1025 -> wt", (2, 1025, 32, 1, 3, 1, 1, 1), (1,), (WT, 0), None),
    ("in1out pads (0,2)", (2, 192, 32, 1, 3, 1, 0, 2), (1,), IN1OUT, None),
    ("in1out pads (2,0)", (2, 192, 32, 1, 3, 1, 2, 0), (1,), IN1OUT, None),
    ("in1out K2", (2, 192, 32, 1, 2, 1, 0, 1), (1,), IN1OUT, None),
    ("wt wide-out 1->64 stride 2", (2, 64, 1, 64, 3, 2, 1, 1), ALL, (WT, 1), None),
    ("wt wide-out 2->32", (2, 64, 2, 32, 3, 1, 1, 1), ALL, (WT, 1), None),
    ("wt wide-in 32->2", (2, 64, 32, 2, 3, 1, 1, 1), ALL, (WT, 0), None),
    ("wt wide-in 32->1 (bf16: in1out)", (2, 64, 32, 1, 3, 1, 1, 1), ALL, {0: (WT, 0), 1: IN1OUT, 2: (WT, 0)}, None),
    ("generic K5 2->2", (2, 40, 2, 2, 5, 1, 2, 2), ALL, GEN, None),
    ("32->24 is not thin: MFMA GEMM", (2, 64, 32, 24, 3, 1, 1, 1), H, GEMM, None),
    ("generic 32->20", (2, 64, 32, 20, 3, 1, 1, 1), H, GEN, None),
    ("generic 12->12", (2, 40, 12, 12, 3, 1, 1, 1), ALL, GEN, None),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_weight_gradient(case):
    G = _G(); c = G.ctx()
    name, shape, dts, spec, ldx = case
    for dt in dts:
        _wgrad(G, c, name, shape, dt, spec, ldx=ldx)
        _wgrad(G, c, name, shape, dt, spec, ldx=ldx, accumulate=True)
    if "65 blocks" in name:
        assert _route(G, 1)["blocks"] >= 64, _route(G, 1)


def test_weight_gradient_bias_by_the_column_sum_kernel(env_switches):
    """tinyv produces db itself; with EEGLDM_NO_FUSED_BIAS_GRAD=1 the column-sum kernel does: same checks, same route"""
    G = _G(); c = G.ctx()
    env_switches(EEGLDM_NO_FUSED_BIAS_GRAD="1")
    for dt in ALL:
        _wgrad(G, c, "tinyv 2->4", (2, 37, 2, 4, 3, 1, 1, 1), dt, (TINYV, 2, 4), tag=" [bias by colsum]")
        _wgrad(G, c, "tinyv 2->4", (2, 37, 2, 4, 3, 1, 1, 1), dt, (TINYV, 2, 4), tag=" [bias by colsum]", accumulate=True)


# the weight-gradient grids are capped at 2 N (tinyv, tiny) and 4 N (wt, generic) blocks
WGRAD_WRAP = [
    ("tinyv", lambda n: (2, n * 256 + 300, 1, 1, 3, 1, 1, 1), 1, (TINYV, 1, 1)),
    ("tiny", lambda n: (2, n * 256 + 300, 3, 3, 3, 1, 1, 1), 1, TINY),
    ("wt", lambda n: (2, 2 * n * 4 + 100, 2, 512, 3, 1, 1, 1), 1, (WT, 1)),
    ("generic", lambda n: (2, 2 * n * 64 + 100, 3, 16, 3, 1, 1, 1), 1, GEN),
]


@pytest.mark.parametrize("case", WGRAD_WRAP, ids=[c[0] for c in WGRAD_WRAP])
def test_weight_gradient_grid_stride_wrap(case):
    """the record proves the wrap (blocks * rows_per_block < rows); the second run proves that the wrapped rows arrive"""
    G = _G(); c = G.ctx()
    name, shape_of, dt, spec = case
    _wgrad(G, c, "wrap " + name, shape_of(_cus()), dt, spec, wrap=True)
    # the bound of a sum over all B Lout rows is wider than the few hundred wrapped rows' whole contribution: a loop that never came round
    # again would pass above.  With dy zero on the rows of the first pass the same bound is that of the wrapped rows alone.
    got = _route(G, 1)
    _wgrad(G, c, "wrap " + name, shape_of(_cus()), dt, spec, wrap=True, keep_from=got["blocks"] * got["rpb"], tag=" [wrapped rows only]")


WGRAD_DET = [
    ("tinyv 2->4", (2, 37, 2, 4, 3, 1, 1, 1), ALL, (TINYV, 2, 4)),
    ("tinyv 65 blocks", (2, 8200, 2, 4, 3, 1, 1, 1), (1,), (TINYV, 2, 4)),
    ("tiny 3->3", (2, 37, 3, 3, 3, 1, 1, 1), ALL, TINY),
    ("in1out 3 segments per sample", (2, 192, 32, 1, 3, 1, 1, 1), (1,), IN1OUT),
    ("wt wide-in 32->2", (2, 64, 32, 2, 3, 1, 1, 1), ALL, (WT, 0)),
    ("wt wide-out 2->32", (2, 64, 2, 32, 3, 1, 1, 1), ALL, (WT, 1)),
    ("generic 12->12", (2, 40, 12, 12, 3, 1, 1, 1), ALL, GEN),
]


@pytest.mark.parametrize("case", WGRAD_DET, ids=[c[0] for c in WGRAD_DET])
def test_weight_gradient_deterministic(case, env_switches):
    """EEGLDM_DETERMINISTIC=1: two runs give dW and db bit for bit, and both pass check A"""
    G = _G(); c = G.ctx()
    env_switches(EEGLDM_DETERMINISTIC="1")
    name, shape, dts, spec = case
    for dt in dts:
        dw1, db1 = _wgrad(G, c, name, shape, dt, spec, tag=" [deterministic, run 1]", det=1)
        dw2, db2 = _wgrad(G, c, name, shape, dt, spec, tag=" [deterministic, run 2]", det=1)
        assert torch.equal(_bits(dw1), _bits(dw2)) and torch.equal(_bits(db1), _bits(db2)), f"{name} [{FMT[dt]}]: two deterministic runs differ"


# ---------------------------------------------------------------------------------------------------------------- non-finite operands
NONFINITE_FWD = [
    ("row 2->4", (2, 19, 2, 4, 3, 1, 1, 1), (ROW, 2, 4)),
    ("in1_seg", (2, 130, 1, 16, 3, 1, 1, 1), SEG),
    ("in1_seg K1 (a tap beyond K must not read the sample)", (2, 130, 1, 16, 1, 1, 0, 0), SEG),
    ("in1_seg stride 2", (2, 300, 1, 64, 3, 2, 1, 1), SEG),
    ("thin_in_reg 2->32", (2, 64, 2, 32, 3, 1, 1, 1), (REG, 2)),
    ("thin_in_reg K1 2->16", (2, 40, 2, 16, 1, 1, 0, 0), (REG, 2)),
    ("thin_in 6->32", (2, 64, 6, 32, 3, 1, 1, 1), LDS),
    ("thin_out_run 32->1", (2, 64, 32, 1, 3, 1, 1, 1), RUN),
    ("thin_out_run K1", (2, 64, 32, 1, 1, 1, 0, 0), RUN),
    ("thin_out 32->3", (2, 64, 32, 3, 3, 1, 1, 1), OUT),
    ("rowdot 24->2", (2, 40, 24, 2, 3, 1, 1, 1), DOT),
    ("point 2->18", (2, 40, 2, 18, 3, 1, 1, 1), PT),
]
NONFINITE_DGRAD = [
    ("row 4->2", (2, 19, 4, 2, 3, 1, 1, 1), (ROW, 2, 4)),
    ("in1_seg 32->1", (2, 130, 32, 1, 3, 1, 1, 1), SEG),
    ("in1_seg K2 16->1 (a tap beyond K must not read the sample)", (2, 130, 16, 1, 2, 1, 0, 1), SEG),
    ("in1_seg K1 16->1", (2, 130, 16, 1, 1, 1, 0, 0), SEG),
    ("thin_in_reg 32->2", (2, 64, 32, 2, 3, 1, 1, 1), (REG, 2)),
    ("thin_in 32->6", (2, 64, 32, 6, 3, 1, 1, 1), LDS),
    ("thin_out 4->64 stride 2", (2, 64, 4, 64, 3, 2, 1, 1), OUT),
    ("rowdot 2->24", (2, 40, 2, 24, 3, 1, 1, 1), DOT),
    ("point K5 3->3", (2, 40, 3, 3, 5, 1, 2, 2), PT),
]
NONFINITE_WGRAD = [
    ("tinyv 2->4", (2, 37, 2, 4, 3, 1, 1, 1), ALL, (TINYV, 2, 4)),
    ("tiny 3->3", (2, 37, 3, 3, 3, 1, 1, 1), ALL, TINY),
    ("in1out 3 segments per sample", (2, 192, 32, 1, 3, 1, 1, 1), (1,), IN1OUT),
    ("wt wide-out 2->32", (2, 64, 2, 32, 3, 1, 1, 1), ALL, (WT, 1)),
    ("wt wide-in 32->2 (inf at x[b, ci, 0]: a clamped tap must not read the sample)", (2, 64, 32, 2, 3, 1, 1, 1), ALL, (WT, 0)),
    ("generic 12->12", (2, 40, 12, 12, 3, 1, 1, 1), ALL, GEN),
]


@pytest.mark.parametrize("case", NONFINITE_FWD, ids=[c[0] for c in NONFINITE_FWD])
def test_forward_nonfinite_input(case):
    """a NaN, a +inf (position 0 of a sample) and a -inf (last position of a sample) in x reach exactly the outputs they feed"""
    G = _G(); c = G.ctx()
    name, shape, spec = case
    for dt in ALL:
        _fwd(G, c, name, shape, dt, spec, ep="b", poison=True, tag=" [NaN/inf in x]")


@pytest.mark.parametrize("case", NONFINITE_DGRAD, ids=[c[0] for c in NONFINITE_DGRAD])
def test_data_gradient_nonfinite_input(case):
    G = _G(); c = G.ctx()
    name, shape, spec = case
    for dt in ALL:
        _dgrad(G, c, name, shape, dt, spec, poison=True, tag=" [NaN/inf in dy]")


@pytest.mark.parametrize("case", NONFINITE_WGRAD, ids=[c[0] for c in NONFINITE_WGRAD])
def test_weight_gradient_nonfinite_input(case):
    G = _G(); c = G.ctx()
    name, shape, dts, spec = case
    for dt in dts:
        for where in ("x", "dy"):
            _wgrad(G, c, name, shape, dt, spec, poison=where)


# ---------------------------------------------------------------------------------------------------------------- fp16 range
F16_RANGE = [
    ("row 2->4", (2, 50, 2, 4, 3, 1, 1, 1), (ROW, 2, 4)),
    ("in1_seg", (2, 130, 1, 16, 3, 1, 1, 1), SEG),
    ("thin_out_run 32->1", (2, 64, 32, 1, 3, 1, 1, 1), RUN),
]


@pytest.mark.parametrize("case", F16_RANGE, ids=[c[0] for c in F16_RANGE])
def test_forward_fp16_range(case):
    """outputs whose RNE(ref) overflows fp16 must be inf (not 65504); outputs in the subnormal range must equal RNE(ref) (not 0).  Weights
    and bias are scaled by 2^15 and 2^-17 as test_gpu_rounding.FWD_EDGE does (no residual: a 16-bit residual at 2^15 would itself hold
    infinities; every weight stays finite, asserted); the shares (> 1e-3 overflow, > 1/2 subnormal) are asserted from the reference before
    the kernel's result is looked at."""
    G = _G(); c = G.ctx()
    name, shape, spec = case
    _fwd(G, c, name, shape, 2, spec, ep="b", scale=2.0 ** 15, tag=" [f16 overflow range]")
    _fwd(G, c, name, shape, 2, spec, ep="b", scale=2.0 ** -17, tag=" [f16 subnormal range]")


# ---------------------------------------------------------------------------------------------------------------- fused LeakyReLU
@pytest.mark.parametrize("L,spec", [(256, SEG), (96, (REG, 1))], ids=["Lo128-in1_seg", "Lo48-thin_in_reg"])
def test_fused_leaky_relu_of_the_discriminator_head(L, spec):
    """The activation fused into the first conv's store is reachable through the discriminator executor only.  Smallest PatchDiscriminator
    the constructor accepts (1 -> 16 channels, stride 2, K 3, one BatchNorm layer); feature 0 = LeakyReLU(conv(x) + b) against
    numerics.conv1d_fwd(..., slope=) with check A (the slope product is one of gamma's four spare roundings).  The family is asserted on a
    plain eegldm_conv1d_fwd of the same shape and leading dimensions (the slope takes no part in the dispatch; after the discriminator's
    forward the record belongs to its later layers)."""
    from eegldm.models import PatchDiscriminator
    G = _G(); c = G.ctx()
    B, C0, slope = 2, 16, float(np.float32(0.2))
    shape = (B, L, 1, C0, 3, 2, 1, 1)
    for dtype, dt in (("float32", 0), ("bfloat16", 1)):
        fmt = FMT[dt]
        _fwd(G, c, f"discriminator head shape L {L}", shape, dt, spec, ep="b")
        net = PatchDiscriminator(num_channels=C0, in_channels=1, out_channels=1, num_layers_d=1, kernel_size=3, padding=1, dtype=dtype)
        x = N.to_storage(_randn((B, 1, L), 91), fmt)
        w = N.to_storage(_randn((C0, 1, 3), 92, 1 / math.sqrt(3)), fmt)
        b = N.rne(_randn((C0,), 93), "f32")
        net.load_state_dict({"initial_conv.conv.weight": w.float(), "initial_conv.conv.bias": b.float()}, strict=False)
        net._forward_native(x.float().to(net.device).contiguous(), 0)
        Cc, Lf = ctypes.c_int(), ctypes.c_int()
        G.check(G.lib.eegldm_disc_feature(net.h, 0, None, ctypes.byref(Cc), ctypes.byref(Lf)))
        assert (Cc.value, Lf.value) == (C0, L // 2)
        f = torch.empty(B, C0, L // 2, device=net.device)
        G.check(G.lib.eegldm_disc_feature(net.h, 0, G.ptr(f), None, None))
        torch.cuda.synchronize()
        ref, mag, emul = N.evaluate(N.conv1d_fwd, x, w, b, 2, 1, 1, slope=slope)
        assert bool((ref < 0).any()) and bool((ref > 0).any())
        N.check(f.cpu(), ref, mag, 3, fmt, emul=emul, route=f"disc feature 0 = lrelu(conv 1->{C0} s2) L {L}")
