"""-m gpu: the GroupNorm kernels of csrc/norm.hip, route by route, against float64 references (tests/numerics.py: gn_stats, gn_fwd, gn_bwd).

Each case names the kernel that must serve its forward and its backward, forces it with the library's switches (env_switches) and confirms
it from eegldm_debug_gn_last_route (family, 4-wide or scalar loads, threads per block, rows-per-thread instantiation, chunk width, XCD-aware
block order); a case served by another kernel fails.  Per case and storage type it prints one `[route]` line per direction and one
`[numerics]` line per check.

What a case checks
  stats    the (mean, rstd) buffer directly against float64: |mean' - mean| <= e_mean, |rstd' / rstd - 1| <= e_rstd (bounds below).  The
           sharp check: it sees a statistics defect before any output rounding hides it.
  forward  check A with d = |gamma| (|xhat| e_rstd + rstd e_mean) + 3u |gamma| rstd (|x| + |mean|) + 4u |z|  (the statistics' error
           carried to z = xhat gamma + beta; the fp32 roundings of the folded scale gamma rstd, of the shift beta - mean gamma rstd and of
           the fma, which act on the UNcentred magnitudes |x| rstd and |mean| rstd; 4 spare roundings), with SiLU 1.1 d + 8u |y| (slope
           <= 1.1, __expf); resampled like the output (both resamples are averages / copies of z, so of d).  And check B.
           xr (resample 1 and 2): one fp32 addition and halving / a copy: check A with 4u |xr|.
  dx       check B against the fp32 autograd emulation (no hard bound is derived for the data gradient).
  dbeta    check A, a plain column sum of the effective upstream gradient over B L terms;  dgamma check A with the statistics' error
           added, as in test_gpu_rounding.py -- both on the SiLU-free cases (with SiLU its derivative at the perturbed z would enter too).

Statistics bounds, from the arithmetic of each route (u = 2^-24, gamma(n) = (n + 4) u, numerics.gamma)
  16-bit resident forward (one pass about a pivot): per thread, in fp32, s1 = sum d and s2 = sum d^2 with d = x - p, p the group's first
      element, over at most n_p = 48 elements (12 rows x 4 channels); fp64 across threads and for mean = p + S1 / n,
      var = S2 / n - (S1 / n)^2.  With m = mean - p:
        e_mean = gamma(n_p) mean|d| + u |mean|
        e_var / var = gamma(n_p + 2) (var + m^2) / var + 2 |m| gamma(n_p) mean|d| / var
        e_rstd = e_var / (2 var) + 8u      (fp32(var), + eps, rsqrtf at 1 ulp, spare)
      The amplification is 1 + m^2 / var with m the distance of ONE sample of the group from its mean: no mean^2 / var term, at any mean.
  split kernels (every type; unchanged): the same one-pass sums about zero, over at most 96 elements per thread: the formulas above
      with p = 0, d = x, m = mean, n_p = 96 -- the 1 + mean^2 / var factor remains THERE (a few 1e-3 of relative rstd error allowed at
      100 sigma).  Giving them the resident kernel's pivot is left for a later change: with it the whole-model bf16 gradient check of
      test_gpu_unet.py drew 1.15 x its storage-gap bound on one tensor (0.90 without), a rounding draw (the mean over all 233 tensors
      moved from 0.60 to 0.63 of the bound, with the pivot in the split kernels alone to 0.59), but a suite that fails is no suite.
  The fp32 engine's arithmetic is unchanged (its outputs stay bit-equal); its flat kernels sum x itself
      (e_mean = gamma(28) mean|x| + u |mean|).
  fp32 resident forward (two passes): s = sum x in fp32 per thread (<= 48), fp64 across; q = sum (x - mean')^2 in fp32 per thread:
        e_mean = gamma(48) mean|x| + u |mean|;   e_rstd = gamma(50) (1 + e_mean^2 / var) / 2 + e_mean^2 / (2 var) + 8u
  flat / wide flat forward, 16-bit types (two passes, fp32 all the way, about the sample's first element p: d = x - p, mean = p + sum d / n, then
      q = sum (d - (mean - p))^2, and xhat = ((x - p) - (mean - p)) rstd): every element passes through at most 12 sequential per-thread
      additions of 8-element trees (3 levels), 6 shuffle levels and the fold of the per-wave sums (<= 6 additions): depth <= 27, so the
      any-order bound holds with n = 28:   e_mean = gamma(28) mean|d| + u |mean|;   e_rstd as for the fp32 resident forward with
      gamma(30) and gamma(28) mean|d| in the place of e_mean.

Inputs: x = scale (randn + offset) rounded to the storage type, offset in units of the standard deviation (0, 30, 100), scale 1 except one
case at 1e-3 (var ~ eps = 1e-6: eps matters) and one at 100 (range); fp16 inputs are asserted finite.  Check B's emulation is torch's fp32
group_norm (+ SiLU, resample) and its autograd on the same operands, as in test_gpu_rounding.py: like the kernels it works on the
uncentred values in fp32, so at a mean of m sigma both carry an absolute error of ~u m in xhat, which the mismatch share of an fp16
output shows (8.9e-3 at 30 sigma for the emulation) -- a centred fp32 formula would be a stricter yardstick than any fp32 kernel that
folds the mean into the shift.  tests/test_groupnorm_numerics_cpu.py holds the fp32 model of the resident arithmetic to the same checks
at 0, 30 and 100 sigma.

Routes and why some have no case
  The forward instantiation for 24 rows per thread was unreachable (resident_chunk never returns more than fwd_rpt_max = 12 rows) and is
  removed.  The XCD-aware order at 1024 threads needs chunks narrower than 128 bytes, which only long rows give: the L = 3072 case.
  The pipelined backward exists for 16-bit types only; the wide flat kernel has no backward (its backward is the split / resident one)."""
import ctypes
import math

import pytest
import torch

import numerics as N

pytestmark = pytest.mark.gpu

FMT = {0: "f32", 1: "bf16", 2: "f16"}
EPS = 1e-6
SPLIT, RESIDENT, PIPE, FLAT, WIDE = 1, 2, 3, 4, 5
FAMILY = {SPLIT: "split", RESIDENT: "resident", PIPE: "pipelined", FLAT: "flat", WIDE: "wide flat"}


def _G():
    import gpu_util as G
    return G


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _route(G_, backward):
    out = (ctypes.c_int * 6)()
    G_.check(G_.lib.eegldm_debug_gn_last_route(backward, out))
    return dict(family=out[0], vec=out[1], nth=out[2], rpt=out[3], cc=out[4], xcd=out[5])


def _confirm(G_, backward, want, name, dt):
    got = _route(G_, backward)
    want = {**{k: v for k, v in want.items() if k != "f32"}, **(want.get("f32", {}) if dt == 0 else {})}
    for k, v in want.items():
        assert got[k] == v, f"{name}: {'backward' if backward else 'forward'} served by {FAMILY.get(got['family'], got['family'])} {got}, expected {k} = {v}"
    print(f"[route] {name} {'bwd' if backward else 'fwd'}: {FAMILY[got['family']]} vec{got['vec']} threads={got['nth']} rows/thread={got['rpt']} "
          f"chunk={got['cc']} xcd={got['xcd']}")


def R(family, **kw):
    return dict(family=family, **kw)


def RES(nth, rpt, cc, xcd, f32=None):
    """a resident launch, named in full; f32: the keys that differ for the fp32 engine"""
    return dict(family=RESIDENT, nth=nth, rpt=rpt, cc=cc, xcd=xcd, **({"f32": f32} if f32 else {}))


NO_NARROW = {"EEGLDM_GN_NO_FEW_SLAB_NARROW": "1"}
NO_PIPE = {"EEGLDM_GN_NO_PIPE": "1"}
UNFENCED = {"EEGLDM_GN_NARROW_UNFENCED": "1"}      # narrow backward blocks are refused while another context of the process is alive: not this test's subject
PIPE_ON = {"EEGLDM_GN_PIPE_MIN_SLABS": "1", "EEGLDM_GN_PIPE_MAX_SLOT": "1"}

# name, (B, L, C, G), dtypes, silu, resample, offset (sigma), scale, options, env, forward route, backward route (None: forward only)
#   options: "ldx2" column view with ld = 2 C, "addend" backward with dxr, "det" deterministic mode too
CASES = [
    # ---- split kernels
    ("split scalar", (2, 50, 6, 3), (0, 1, 2), 1, 0, 30.0, 1.0, "", {}, R(SPLIT, vec=0), R(SPLIT, vec=0)),
    ("split 4-wide (resident off)", (2, 100, 64, 8), (0, 1, 2), 0, 0, 100.0, 1.0, "det", {"EEGLDM_GN_NO_RESIDENT": "1"}, R(SPLIT, vec=1), R(SPLIT, vec=1)),
    ("split 4-wide avgpool, xr", (2, 100, 64, 8), (1, 2), 1, 1, 30.0, 1.0, "addend", {"EEGLDM_GN_NO_RESIDENT": "1"}, R(SPLIT, vec=1), R(SPLIT, vec=1)),
    ("split scalar nearest x2, xr", (2, 50, 6, 3), (0, 1), 0, 2, 0.0, 1.0, "addend", {}, R(SPLIT, vec=0), R(SPLIT, vec=0)),
    # ---- resident, 1024 threads (the production launch): both rows-per-thread instantiations.  RES(threads, rows per thread, chunk, xcd);
    #      f32 = what differs for the fp32 engine (its backward holds 4 or 8 rows per thread, so its chunks are narrower)
    ("resident 1024 R6", (8, 96, 256, 32), (0, 1, 2), 0, 0, 30.0, 1.0, "det", {**NO_NARROW, **NO_PIPE},
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    ("resident 1024 R12", (8, 192, 256, 32), (0, 1, 2), 1, 0, 100.0, 1.0, "", {**NO_NARROW, **NO_PIPE},
     RES(1024, 12, 256, 0), RES(1024, 12, 256, 0, f32=dict(rpt=8, cc=128))),
    ("resident 1024 plain order (the finding's shape)", (4, 192, 256, 32), (1, 2), 0, 0, 30.0, 1.0, "", NO_NARROW,
     RES(1024, 12, 256, 0), RES(1024, 12, 256, 0)),
    ("resident 1024 row tail L100", (4, 100, 256, 32), (0, 1, 2), 1, 0, 30.0, 1.0, "addend", NO_NARROW,
     RES(1024, 12, 256, 0), RES(1024, 12, 256, 0, f32=dict(rpt=8))),
    ("resident 1024 cpg L = 1024 (exact reciprocal)", (4, 128, 256, 32), (1, 2), 0, 0, 100.0, 1.0, "", NO_NARROW,
     RES(1024, 12, 256, 0), RES(1024, 12, 256, 0)),
    ("resident 1024 XCD order L3072", (8, 3072, 64, 16), (0, 1, 2), 0, 0, 30.0, 1.0, "", NO_NARROW,
     RES(1024, 12, 16, 1), RES(1024, 12, 16, 1, f32=dict(rpt=8, cc=8))),
    ("resident 1024 |x| 1e-3 (eps)", (8, 96, 256, 32), (0, 1, 2), 0, 0, 0.0, 1e-3, "", {**NO_NARROW, **NO_PIPE},
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    ("resident 1024 |x| 100 (range)", (8, 96, 256, 32), (0, 1, 2), 1, 0, 0.0, 100.0, "", {**NO_NARROW, **NO_PIPE},
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    # ---- resident, narrower blocks
    ("resident 512", (8, 96, 256, 32), (0, 1, 2), 0, 0, 100.0, 1.0, "", {"EEGLDM_GN_FWD_NTH": "512", "EEGLDM_GN_BWD_NTH": "512", **UNFENCED, **NO_PIPE},
     RES(512, 12, 256, 1), RES(512, 12, 256, 1, f32=dict(rpt=8, cc=128))),
    ("resident 256", (8, 96, 256, 32), (0, 1, 2), 1, 0, 30.0, 1.0, "addend", {"EEGLDM_GN_FWD_NTH": "256", "EEGLDM_GN_BWD_NTH": "256", **UNFENCED, **NO_PIPE},
     RES(256, 12, 128, 1), RES(256, 12, 128, 1, f32=dict(rpt=8, cc=64))),
    ("resident few-slab narrowing B1 (default switches)", (1, 192, 256, 32), (0, 1, 2), 0, 0, 100.0, 1.0, "", {},
     RES(256, 12, 64, 0), RES(1024, 12, 256, 0, f32=dict(rpt=8, cc=128))),
    # ---- resident, resample / views
    ("resident avgpool (pair mode), xr", (8, 96, 256, 32), (0, 1, 2), 1, 1, 30.0, 1.0, "addend", NO_NARROW,
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    ("resident nearest x2, xr", (8, 96, 256, 32), (0, 1, 2), 0, 2, 30.0, 1.0, "addend det", NO_NARROW,
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    ("resident column view ld = 2 C", (8, 96, 256, 32), (0, 1, 2), 0, 0, 30.0, 1.0, "ldx2", {**NO_NARROW, **NO_PIPE},
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0, f32=dict(rpt=8))),
    # ---- pipelined persistent backward (16-bit only), one slot per XCD
    ("pipelined bwd 256-channel slabs", (8, 96, 256, 32), (1, 2), 0, 0, 30.0, 1.0, "", {**NO_NARROW, **PIPE_ON},
     RES(1024, 6, 256, 0), R(PIPE, nth=1024, rpt=6, cc=256, xcd=1)),
    ("pipelined bwd 64-channel slabs, SiLU", (8, 384, 64, 16), (1, 2), 1, 0, 30.0, 1.0, "", {**NO_NARROW, **PIPE_ON},
     RES(1024, 6, 64, 0), R(PIPE, nth=1024, rpt=6, cc=64, xcd=1)),
    ("pipelined bwd 128-channel slabs, addend", (16, 192, 128, 32), (1, 2), 0, 0, 100.0, 1.0, "addend det",
     {**NO_NARROW, **PIPE_ON, "EEGLDM_GN_PIPE_ADDEND": "1"}, RES(1024, 6, 128, 0), R(PIPE, nth=1024, rpt=6, cc=128, xcd=1)),
    ("pipelined bwd gate: B4 falls back", (4, 96, 256, 32), (1,), 0, 0, 30.0, 1.0, "", {**NO_NARROW, **PIPE_ON},
     RES(1024, 6, 256, 0), RES(1024, 6, 256, 0)),
    # ---- flat G = 1 kernels: 3-chunk and 12-chunk instantiations, and one element row past the limit
    ("flat C1 n6144", (3, 6144, 1, 1), (0, 1, 2), 1, 0, 30.0, 1.0, "", {}, R(FLAT, rpt=3, cc=1), R(FLAT, rpt=3, cc=1)),
    ("flat C1 n24576", (3, 24576, 1, 1), (1, 2), 0, 0, 100.0, 1.0, "", {}, R(FLAT, rpt=12, cc=1), R(FLAT, rpt=12, cc=1)),
    ("flat C2 n6144", (3, 3072, 2, 1), (1, 2), 1, 0, 30.0, 1.0, "", {}, R(FLAT, rpt=3, cc=2), R(FLAT, rpt=3, cc=2)),
    ("flat C2 n24576", (3, 12288, 2, 1), (1, 2), 0, 0, 100.0, 1.0, "addend", {}, R(FLAT, rpt=12, cc=2), R(FLAT, rpt=12, cc=2)),
    ("flat C4 n6144", (3, 1536, 4, 1), (1, 2), 0, 0, 0.0, 1.0, "det", {}, R(FLAT, rpt=3, cc=4), R(FLAT, rpt=3, cc=4)),
    ("flat C4 n24576", (3, 6144, 4, 1), (0, 1, 2), 1, 0, 30.0, 1.0, "addend", {}, R(FLAT, rpt=12, cc=4), R(FLAT, rpt=12, cc=4)),
    ("flat C8 n6144", (3, 768, 8, 1), (1, 2), 0, 0, 100.0, 1.0, "", {}, R(FLAT, rpt=3, cc=8), R(FLAT, rpt=3, cc=8)),
    ("flat C8 n24576", (3, 3072, 8, 1), (0, 1, 2), 1, 0, 30.0, 1.0, "", {}, R(FLAT, rpt=12, cc=8), R(FLAT, rpt=12, cc=8)),
    ("flat limit: n24584 falls back", (2, 3073, 8, 1), (1,), 0, 0, 30.0, 1.0, "", {}, R(SPLIT, vec=1), R(SPLIT, vec=1)),
    ("flat off", (3, 3072, 8, 1), (1,), 0, 0, 30.0, 1.0, "", {"EEGLDM_GN_NO_FLAT": "1"}, R(SPLIT, vec=1), R(SPLIT, vec=1)),
    # ---- wide flat forward: both chunk instantiations; fp32 only up to 6 chunks
    ("wide flat C16 n49152", (2, 3072, 16, 1), (0, 1, 2), 1, 0, 30.0, 1.0, "", {}, R(WIDE, rpt=6, cc=16), None),
    ("wide flat C16 n98304", (2, 6144, 16, 1), (1, 2), 0, 0, 100.0, 1.0, "", {}, R(WIDE, rpt=12, cc=16), None),
    ("wide flat C64 n49152", (2, 768, 64, 1), (1, 2), 0, 0, 0.0, 1.0, "", {}, R(WIDE, rpt=6, cc=64), None),
    ("wide flat C64 n98304", (2, 1536, 64, 1), (1, 2), 1, 0, 30.0, 1.0, "", {}, R(WIDE, rpt=12, cc=64), None),
    ("wide flat fp32 size gate: n98304 falls back", (2, 1536, 64, 1), (0,), 0, 0, 30.0, 1.0, "", {}, R(SPLIT, vec=1), None),
]


def _stat_bounds(x, G, fam, fmt):
    """(mean, var, rstd, e_mean, e_rstd), each (B, G) float64: the bounds of the module docstring for the route family and storage type"""
    B = x.shape[0]
    xg = x.reshape(B, G, -1)
    mean, var, rstd = N.gn_stats(x, G, EPS)
    u = N.U32
    if fmt != "f32" and fam in (RESIDENT, PIPE):
        n_p = 48
        d = xg - xg[:, :, :1]
        m = d.mean(-1); mad = d.abs().mean(-1)
        em = N.gamma(n_p) * mad + u * mean.abs()
        ev = N.gamma(n_p + 2) * (var + m ** 2) / var + 2 * m.abs() * N.gamma(n_p) * mad / var
        return mean, var, rstd, em, 0.5 * ev + 8 * u
    if fam == SPLIT:        # one-pass sums about zero, every type
        mad = xg.abs().mean(-1)
        em = N.gamma(96) * mad + u * mean.abs()
        ev = N.gamma(98) * (var + mean ** 2) / var + 2 * mean.abs() * N.gamma(96) * mad / var
        return mean, var, rstd, em, 0.5 * ev + 8 * u
    if fam == RESIDENT:
        em0 = N.gamma(48) * xg.abs().mean(-1); n_q = 50
    elif fmt == "f32":
        em0 = N.gamma(28) * xg.abs().mean(-1); n_q = 30
    else:
        em0 = N.gamma(28) * (xg - xg[:, :, :1]).abs().mean(-1); n_q = 30
    er = 0.5 * N.gamma(n_q) * (1 + em0 ** 2 / var) + 0.5 * em0 ** 2 / var + 8 * u
    return mean, var, rstd, em0 + u * mean.abs(), er


def _dy_eff(dy, resample):
    """the gradient that reaches z: the transpose of numerics.gn_resample"""
    if resample == 1:
        return 0.5 * dy.repeat_interleave(2, dim=2)
    if resample == 2:
        return dy[:, :, 0::2] + dy[:, :, 1::2]
    return dy


def _buf(G_, rows, C, ld, dt):
    """device [rows, ld] buffer (NaN-filled so that an unwritten element shows) and its [rows, C] view"""
    t = torch.full((rows, ld), math.nan, device=G_.DEV, dtype=G_.TDT[dt])
    return t, t[:, :C]


def _run_case(G_, c, case, dt, env_switches, poison=None, twice=False):
    """forward, then the backward once per mode (default; deterministic twice more on a "det" case).  twice: default and deterministic mode,
    each backward run a second time right behind the first (dgamma, dbeta zeroed, dx NaN-filled again): the SECOND call's results are returned"""
    name, (B, L, C, Gr), _dts, silu, rs, off, scale, opts, env, want_f, want_b = case
    fmt = FMT[dt]; tag = f"{name} [{fmt}]"
    env_switches(**env)
    Lo = L // 2 if rs == 1 else (2 * L if rs == 2 else L)
    x = N.to_storage(scale * (_randn((B, C, L), 71) + off), fmt)
    if poison:
        for idx, v in poison:
            x[idx] = v
    else:
        assert bool(torch.isfinite(x).all()), tag
    ga = N.rne(1 + 0.1 * _randn((C,), 72), "f32"); be = N.rne(0.1 * _randn((C,), 73), "f32")
    dy = N.to_storage(_randn((B, C, Lo), 74), fmt)
    dxr = N.to_storage(_randn((B, C, Lo), 75), fmt) if "addend" in opts else None
    ld = 2 * C if "ldx2" in opts else C
    xd = G_.nlc(x, dt, ld=ld); gad, bed = ga.float().to(G_.DEV), be.float().to(G_.DEV)
    yb, yd = _buf(G_, B * Lo, C, C, dt)
    st = torch.full((B * Gr * 2,), math.nan, device=G_.DEV)
    xrb = _buf(G_, B * Lo, C, C, dt)[0] if rs else None
    G_.check(G_.lib.eegldm_groupnorm_fwd(c.h, G_.ptr(xd), ld, G_.ptr(gad), G_.ptr(bed), G_.ptr(yb), C, G_.ptr(st), B, L, C, Gr, EPS, silu, rs,
                                         G_.ptr(xrb) if rs else None, C if rs else 0, dt))
    torch.cuda.synchronize()
    _confirm(G_, 0, want_f, tag, dt)
    out = dict(x=x, ga=ga, be=be, dy=dy, dxr=dxr, y=G_.ncl(yd, B, Lo).double(), st=st.cpu().double().reshape(B, Gr, 2),
               xr=G_.ncl(xrb, B, Lo).double() if rs else None)
    if want_b is None:
        return out
    dyd = G_.nlc(dy, dt); dxrd = G_.nlc(dxr, dt) if dxr is not None else None
    runs = []
    for det in ((None, "1") if twice else (None, "1", "1") if "det" in opts else (None,)):
        env_switches(EEGLDM_DETERMINISTIC=det)
        dxb, dxd = _buf(G_, B * L, C, C, dt)
        dga = torch.zeros(C, device=G_.DEV); dbe = torch.zeros(C, device=G_.DEV)
        for call in range(2 if twice else 1):
            if call:
                dxb.fill_(math.nan); dga.zero_(); dbe.zero_()
            G_.check(G_.lib.eegldm_groupnorm_bwd(c.h, G_.ptr(xd), ld, G_.ptr(gad), G_.ptr(bed), G_.ptr(st), G_.ptr(dyd), C, G_.ptr(dxb), C,
                                                 G_.ptr(dga), G_.ptr(dbe), B, L, C, Gr, silu, rs, G_.ptr(dxrd) if dxrd is not None else None,
                                                 C if dxrd is not None else 0, dt))
            torch.cuda.synchronize()
            _confirm(G_, 1, want_b, tag + (" deterministic" if det else "") + (" second call" if call else ""), dt)
        runs.append(dict(det=bool(det), dx=G_.ncl(dxd, B, L).double(), dga=dga.cpu().double(), dbe=dbe.cpu().double()))
    env_switches(EEGLDM_DETERMINISTIC=None)
    out["bwd"] = runs
    return out


def _ids(cases):
    return [c[0] for c in cases]


def _check_backward(o, runs, case, fmt, stats, tag):
    """the backward checks of the module docstring on every run of `runs`; stats = (mean, rstd, e_mean, e_rstd) of _stat_bounds"""
    name, (B, L, C, Gr), _dts, silu, rs, _off, _scale, _opts, _env, _want_f, _want_b = case
    x, ga, be, dy, dxr = o["x"], o["ga"], o["be"], o["dy"], o["dxr"]
    mean, rstd, em, er = stats
    rep = lambda t: t.repeat_interleave(C // Gr, dim=1)[:, :, None]
    xhat = (x - rep(mean)) * rep(rstd)
    dx_ref, dga_ref, dbe_ref = N.gn_bwd(x, Gr, ga, be, dy, EPS, silu, rs, dxr)
    dx_em, _g, _b = N.gn_bwd(x.float(), Gr, ga.float(), be.float(), dy.float(), EPS, silu, rs, dxr.float() if dxr is not None else None, torch_norm=True)
    de = _dy_eff(dy, rs)
    for r in runs:
        mode = " det" if r["det"] else ""
        if fmt != "f32":
            N.check_b(r["dx"], dx_ref, dx_em, fmt, route=tag + " dx" + mode)
        else:
            # fp32 data gradient: no rounding cell to take statistics of.  dx = rstd (dz gamma - m1 - xhat m2) is linear in dz with
            # coefficients made of rstd and xhat, which the kernel holds to e_rstd and |xhat| e_rstd + rstd e_mean; three such terms with
            # |xhat| <= 8, and the fp32 group sums m1, m2 over cpg L elements: relative to max |dx|
            tol = 3 * 9 * float((er + rstd * em).max()) + N.gamma(C // Gr * L)
            err = float((r["dx"] - dx_ref).abs().max() / dx_ref.abs().max())
            print(f"[numerics] {tag} dx{mode}: max error {err:.2e} of max |dx| (bound {tol:.2e})")
            assert err <= tol, f"{tag} dx{mode}: {err:.3e} > {tol:.3e}"
        if not silu:
            N.check(r["dbe"], dbe_ref, de.abs().sum((0, 2)), B * L, "f32", route=tag + " dbeta" + mode)
            dgd = N.gamma(B * L) * (de * xhat).abs().sum((0, 2)) + (de.abs() * (xhat.abs() * rep(er) + rep(rstd) * rep(em))).sum((0, 2))
            N.check(r["dga"], dga_ref, dgd / N.gamma(0), 0, "f32", route=tag + " dgamma" + mode)


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_groupnorm_route_against_float64(case, env_switches):
    G_ = _G(); c = G_.ctx()
    name, (B, L, C, Gr), dts, silu, rs, off, scale, opts, env, want_f, want_b = case
    rep = lambda t: t.repeat_interleave(C // Gr, dim=1)[:, :, None]
    u = N.U32
    for dt in dts:
        fmt = FMT[dt]; tag = f"{name} [{fmt}]"
        o = _run_case(G_, c, case, dt, env_switches)
        x, ga, be, dy, dxr = o["x"], o["ga"], o["be"], o["dy"], o["dxr"]
        mean, var, rstd, em, er = _stat_bounds(x, Gr, want_f["family"], fmt)
        # ---- statistics
        e_m = ((o["st"][:, :, 0] - mean).abs() / em).max().item(); e_r = ((o["st"][:, :, 1] / rstd - 1).abs() / er).max().item()
        print(f"[numerics] {tag} stats: mean error {e_m:.3f} x bound (bound / std {float((em * rstd).max()):.2e}), rstd error {e_r:.3f} x bound "
              f"(bound {float(er.max()):.2e}), mean^2 / var up to {float((mean ** 2 / var).max()):.3g}")
        assert e_m <= 1 and e_r <= 1, f"{tag}: statistics outside their bound (mean {e_m:.3g} x, rstd {e_r:.3g} x)"
        # ---- forward
        ref = N.gn_fwd(x, Gr, ga, be, EPS, silu, rs)
        emul = N.gn_fwd(x.float(), Gr, ga.float(), be.float(), EPS, silu, rs, torch_norm=True)
        xhat = (x - rep(mean)) * rep(rstd)
        z = xhat * ga[:, None] + be[:, None]
        d = ga.abs()[:, None] * (xhat.abs() * rep(er) + rep(rstd) * rep(em)) + 3 * u * ga.abs()[:, None] * rep(rstd) * (x.abs() + rep(mean).abs()) \
            + 4 * u * z.abs()
        d = N.gn_resample(d, rs)
        if silu:
            d = 1.1 * d + 8 * u * ref.abs()
        N.check(o["y"], ref, d / N.gamma(0), 0, fmt, route=tag + " fwd A", min_stat=math.inf)
        if fmt != "f32":
            N.check_b(o["y"], ref, emul, fmt, route=tag + " fwd B")
        if rs:
            xr_ref = N.gn_xr(x, rs)
            N.check(o["xr"], xr_ref, xr_ref.abs(), 0, fmt, route=tag + " xr")
        if want_b is None:
            continue
        _check_backward(o, o["bwd"][:2], case, fmt, (mean, rstd, em, er), tag)
        dets = [r for r in o["bwd"] if r["det"]]
        if len(dets) == 2:
            for k in ("dx", "dga", "dbe"):
                assert torch.equal(dets[0][k], dets[1][k]), f"{tag}: {k} differs between two deterministic-mode runs"
            print(f"[numerics] {tag}: dx, dgamma, dbeta bit-equal across two deterministic-mode runs")


def _pattern(got, ref, what):
    ng, nr = ~torch.isfinite(got.double()), ~torch.isfinite(ref.double())
    assert bool(nr.any()), f"{what}: the reference has no non-finite element"
    bad = ng != nr
    assert not bool(bad.any()), f"{what}: non-finite pattern differs in {int(bad.sum())} of {ref.numel()} elements (kernel {int(ng.sum())}, " \
                                f"reference {int(nr.sum())} non-finite)"
    print(f"[nonfinite] {what}: {int(nr.sum())} non-finite elements, same pattern as the reference")


NONFINITE = [c for c in CASES if c[0] in ("resident 1024 R6", "pipelined bwd 256-channel slabs", "flat C8 n24576", "split 4-wide (resident off)")]


@pytest.mark.parametrize("case", NONFINITE, ids=_ids(NONFINITE))
def test_second_backward_call_holds_the_first_call_bounds(case, env_switches):
    """The dgamma / dbeta slot areas are shared between launches and re-zeroed by the fold that follows each launch; a launch whose partials
    go to one area and whose fold reads (or clears) another is right once and wrong from the next call on.  One case per backward family
    (split, resident, pipelined, flat), in the default and in the deterministic mode: the backward runs twice in a row, dgamma and dbeta
    zeroed in between, and the SECOND call's dx, dgamma and dbeta are held to the bounds of the first."""
    G_ = _G(); c = G_.ctx()
    name, (B, L, C, Gr), dts, silu, rs, off, scale, opts, env, want_f, want_b = case
    for dt in dts:
        fmt = FMT[dt]; tag = f"{name} [{fmt}] second call"
        o = _run_case(G_, c, case, dt, env_switches, twice=True)
        mean, _var, rstd, em, er = _stat_bounds(o["x"], Gr, want_f["family"], fmt)
        assert [r["det"] for r in o["bwd"]] == [False, True], tag
        _check_backward(o, o["bwd"], case, fmt, (mean, rstd, em, er), tag)


@pytest.mark.parametrize("case", NONFINITE, ids=_ids(NONFINITE))
def test_nonfinite_x_reaches_its_group(case, env_switches):
    """A NaN (inside a group, off the pivot element) and an inf (ON the first element of another sample's group, the pivot of the one-pass
    statistics) in x must make exactly the elements non-finite that they make non-finite in float64: the whole (sample, group) in the
    forward and in dx, and -- through the stored statistics -- the group's channels of dgamma (and of dbeta where SiLU's derivative enters)."""
    G_ = _G(); c = G_.ctx()
    name, (B, L, C, Gr), dts, silu, rs, off, scale, opts, env, want_f, want_b = case
    cpg = C // Gr
    spots = [((0, min(C - 1, cpg + 1), 5), math.nan), ((B - 1, (Gr - 1) * cpg, 0), math.inf)]
    for dt in [d for d in dts if d != 0]:
        tag = f"{name} [{FMT[dt]}]"
        o = _run_case(G_, c, case, dt, env_switches, poison=spots)
        x, ga, be, dy, dxr = o["x"], o["ga"], o["be"], o["dy"], o["dxr"]
        _pattern(o["y"], N.gn_fwd(x, Gr, ga, be, EPS, silu, rs), tag + " forward")
        mean, _var, rstd = N.gn_stats(x, Gr, EPS)
        _pattern(o["st"][:, :, 1], rstd, tag + " rstd")
        dx_ref, dga_ref, dbe_ref = N.gn_bwd(x, Gr, ga, be, dy, EPS, silu, rs, dxr)
        r = o["bwd"][0]
        _pattern(r["dx"], dx_ref, tag + " dx")
        _pattern(r["dga"], dga_ref, tag + " dgamma")
        if silu:
            _pattern(r["dbe"], dbe_ref, tag + " dbeta")
        else:
            assert bool(torch.isfinite(r["dbe"]).all()) and bool(torch.isfinite(dbe_ref).all()), tag + " dbeta"
