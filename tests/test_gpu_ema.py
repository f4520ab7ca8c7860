"""-m gpu: the weight EMA -- fused Adam + EMA kernel against the composed form (bit for bit) and against a float64 recurrence,
GradScaler skips, EMA.applied() (weights and every derived copy), determinism, and the entry scripts' checkpoints."""
import os

import numpy as np
import pytest
import torch

from make_golden_cases import UNET_CASES
from param_gen import gen_param, normal, timesteps

pytestmark = pytest.mark.gpu

N_FULL = 30537731          # parameters of the config_ldm UNet
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)


def ema_reference_f64(e64, p32, c32):
    """One EMA update in float64 with the float32-rounded constant the kernel receives."""
    e64 += float(np.float32(c32)) * (p32.double() - e64)
    return e64


def _views(n, offsets, seed):
    """Five random buffers of n floats, buffer k starting `offsets[k]` floats into a 16-byte aligned allocation, guard values around."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    bufs, views = [], []
    for k, off in enumerate(offsets):
        b = torch.randn(n + 16, device="cuda", generator=g)
        if k == 3:
            b = b.abs()                      # second moment
        assert b.data_ptr() % 16 == 0
        bufs.append(b); views.append(b[off:off + n])
    return bufs, views


@pytest.mark.parametrize("n", [1, 3, 4, 1023, N_FULL])
@pytest.mark.parametrize("offsets", [(1, 1, 1, 1, 1), (0, 0, 0, 0, 0), (3, 3, 3, 3, 3), (1, 2, 0, 3, 2)],
                         ids=["off4B", "aligned", "off12B", "mixed"])
def test_fused_equals_composed_bit_for_bit(n, offsets):
    """adam_step_ema == adam_step for p, m, v and == adam_step + ema_update for the shadow; buffers at a 4-byte but not 16-byte aligned
    address (scalar head + float4 body + scalar tail), aligned, and with different misalignments (all-scalar route).  Nothing outside
    [0, n) is written."""
    import gpu_util as G
    c = G.ctx()
    step, ginv, omd = 7, 1.0 / 1024.0, float(np.float32(1.0 - 0.9993))
    bufs_a, (p, g, m, v, e) = _views(n, offsets, seed=n % 1000 + 1)
    bufs_b = [b.clone() for b in bufs_a]
    p2, g2, m2, v2, e2 = (b[off:off + n] for b, off in zip(bufs_b, offsets))
    before = [b.clone() for b in bufs_a]
    G.check(G.lib.eegldm_adam_step_ema(c.h, G.ptr(p), G.ptr(g), G.ptr(m), G.ptr(v), G.ptr(e), n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"],
                                       step, ginv, omd))
    G.check(G.lib.eegldm_adam_step(c.h, G.ptr(p2), G.ptr(g2), G.ptr(m2), G.ptr(v2), n, ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], step, ginv))
    G.check(G.lib.eegldm_ema_update(c.h, G.ptr(e2), G.ptr(p2), n, omd))
    torch.cuda.synchronize()
    for name, a, b in zip("pgmve", bufs_a, bufs_b):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: fused != composed (n={n}, offsets={offsets})"
    for name, a, b0, off in zip("pgmve", bufs_a, before, offsets):
        assert torch.equal(a[:off], b0[:off]) and torch.equal(a[off + n:], b0[off + n:]), f"{name}: written outside the range"
        if name != "g":
            assert not torch.equal(a[off:off + n], b0[off:off + n]), f"{name}: not updated"
    # the shadow really is fma(c, p - e, e) of the NEW parameters (float64 check of the first elements; bound: one rounding each in p - e and the fma)
    k = min(n, 4096)
    off_p, off_e = offsets[0], offsets[4]
    e_old, p_new, e_new = before[4][off_e:off_e + k], bufs_a[0][off_p:off_p + k], bufs_a[4][off_e:off_e + k]
    want = ema_reference_f64(e_old.double().clone(), p_new, omd)
    bound = 2.0 ** -24 * (want.abs() + omd * (p_new.double() - e_old.double()).abs()) + 1e-45
    assert bool(((e_new.double() - want).abs() <= bound).all())


@pytest.mark.parametrize("n", [1, 3, 4, 1023, N_FULL])
@pytest.mark.parametrize("offs", [(1, 1), (0, 0), (2, 3)], ids=["off4B", "aligned", "mixed"])
def test_swap_exchanges_and_twice_is_identity(n, offs):
    import gpu_util as G
    c = G.ctx()
    g = torch.Generator(device="cuda").manual_seed(n % 1000 + 5)
    A, B = torch.randn(n + 16, device="cuda", generator=g), torch.randn(n + 16, device="cuda", generator=g)
    A0, B0 = A.clone(), B.clone()
    a, b = A[offs[0]:offs[0] + n], B[offs[1]:offs[1] + n]
    G.check(G.lib.eegldm_swap(c.h, G.ptr(a), G.ptr(b), n))
    assert torch.equal(a, B0[offs[1]:offs[1] + n]) and torch.equal(b, A0[offs[0]:offs[0] + n])
    assert torch.equal(A[:offs[0]], A0[:offs[0]]) and torch.equal(A[offs[0] + n:], A0[offs[0] + n:])
    assert torch.equal(B[:offs[1]], B0[:offs[1]]) and torch.equal(B[offs[1] + n:], B0[offs[1] + n:])
    G.check(G.lib.eegldm_swap(c.h, G.ptr(a), G.ptr(b), n))
    assert torch.equal(A.view(torch.int32), A0.view(torch.int32)) and torch.equal(B.view(torch.int32), B0.view(torch.int32))


def test_nan_and_inf_parameters_reach_the_shadow():
    import gpu_util as G
    c = G.ctx()
    p = torch.tensor([float("nan"), float("inf"), -float("inf"), 1.0, 2.0, 3.0, float("nan")], device="cuda")
    e = torch.zeros(7, device="cuda")
    G.check(G.lib.eegldm_ema_update(c.h, G.ptr(e), G.ptr(p), 7, 0.25))
    assert torch.isnan(e[0]) and e[1] == float("inf") and e[2] == -float("inf") and torch.isnan(e[6])
    assert e[3:6].tolist() == [0.25, 0.5, 0.75]


def _tiny_unet(dtype="float32", seed=7, **extra):
    from eegldm.models import UNetModel
    cfg = dict(UNET_CASES["tiny_l64"][0], **extra)
    net = UNetModel(**cfg, dtype=dtype)
    sd = {k: torch.from_numpy(gen_param(seed, k, tuple(v.shape))) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    return net, cfg


def _train_steps(net, opt, n_steps, first=0, scaler=None, after=None):
    from eegldm.schedulers import DDPMScheduler
    from eegldm.training import ldm_train_step
    sched = DDPMScheduler(num_train_timesteps=1000, schedule="scaled_linear_beta", beta_start=0.0015, beta_end=0.0195)
    B, L = 2, 64
    dev = net.device
    for i in range(first, first + n_steps):
        lat = torch.from_numpy(normal((B, 1, L), seed=100 + i)).to(dev); nz = torch.from_numpy(normal((B, 1, L), seed=500 + i)).to(dev)
        t = torch.from_numpy(timesteps(B, seed=900 + i)).to(dev)
        net.train(); opt.zero_grad()
        ldm_train_step(net, sched, lat, nz, t, grad_scale=scaler.get_scale() if scaler else 1.0)
        if scaler:
            scaler.step(opt); scaler.update()
        else:
            opt.step()
        if after:
            after(i)


@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "constant"])
def test_shadow_against_float64_recurrence(warmup):
    """200 fused updates on a small UNet driven by real train steps, against e += c32 * (p - e) in float64 with the same float32 constant.
    Bound (derived, nothing added): an update commits at most one rounding in p - e (relative 2^-24, and it enters the result times c) and
    one in the fma (relative 2^-24 of the new e); the recurrence scales an existing error by 1 - c <= 1.  After N updates
    |e32 - e64| <= N * 2^-24 * (max|e| + c_max * max|p - e|), maxima over elements and trajectory."""
    from eegldm.training import Adam, EMA
    net, _ = _tiny_unet()
    ema = EMA(net, decay=0.999, warmup=warmup)
    opt = Adam(net, lr=1e-4, ema=ema)
    e64 = net.flat.double().clone()
    st = dict(max_e=float(e64.abs().max()), max_d=0.0, c_max=0.0, n=0)

    def after(_i):
        c32 = float(np.float32(1.0 - ema.decay_at(st["n"])))
        st["max_d"] = max(st["max_d"], float((net.flat.double() - e64).abs().max()))
        ema_reference_f64(e64, net.flat, c32)
        st["max_e"] = max(st["max_e"], float(e64.abs().max())); st["c_max"] = max(st["c_max"], c32); st["n"] += 1

    N = 200
    _train_steps(net, opt, N, after=after)
    assert ema.num_updates == N == st["n"] and opt.step_count == N
    err = float((ema.shadow.double() - e64).abs().max())
    bound = N * 2.0 ** -24 * (st["max_e"] + st["c_max"] * st["max_d"])
    print(f"warmup={warmup}: max|e32 - e64| {err:.3e}, bound {bound:.3e}, max|e| {st['max_e']:.3e}, max|p-e| {st['max_d']:.3e}, c_max {st['c_max']:.3e}")
    assert st["max_d"] > 0 and not torch.equal(ema.shadow, net.flat)
    assert err <= bound
    # the stand-alone update follows the same recurrence
    ema.update()
    ema_reference_f64(e64, net.flat, 1.0 - ema.decay_at(N))
    assert ema.num_updates == N + 1 and float((ema.shadow.double() - e64).abs().max()) <= (N + 1) * 2.0 ** -24 * (st["max_e"] + st["c_max"] * st["max_d"])


def test_grad_scaler_skip_leaves_the_ema_alone():
    from eegldm.training import Adam, EMA, GradScaler
    net, _ = _tiny_unet()
    ema = EMA(net, decay=0.9, warmup=False)
    opt = Adam(net, lr=1e-3, ema=ema)
    scaler = GradScaler(init_scale=1024.0)
    _train_steps(net, opt, 2, scaler=scaler)
    assert ema.num_updates == 2 and opt.step_count == 2
    snap = [t.clone() for t in (net.flat, opt.m, opt.v, ema.shadow)]
    net.flat_grad[5] = float("inf")
    assert scaler.step(opt) is None
    scaler.update()
    assert scaler.get_scale() == 512.0 and ema.num_updates == 2 and opt.step_count == 2
    for a, b in zip((net.flat, opt.m, opt.v, ema.shadow), snap):
        assert torch.equal(a, b)
    _train_steps(net, opt, 1, first=2, scaler=scaler)
    assert ema.num_updates == 3 and opt.step_count == 3
    for a, b in zip((net.flat, opt.m, opt.v, ema.shadow), snap):
        assert not torch.equal(a, b)


BIG = dict(in_channels=1, out_channels=1, model_channels=128, num_res_blocks=1, attention_resolutions=[4], channel_mult=[1, 2, 4], resblock_updown=True)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("B", [1, 8], ids=["b1_few_rows", "b8_big_tiles"])
def test_applied_swaps_every_weight_copy(dtype, B, env_switches):
    """Inside applied() the model computes exactly what a FRESH model loaded from ema.state_dict() computes (a derived weight copy that
    sync_weights() missed would show here), and the raw weights -- flat buffer and copies -- are back afterwards."""
    from eegldm.models import UNetModel
    from eegldm.training import EMA
    if B > 1:
        env_switches(EEGLDM_GEMM_BIG_MIN_TILES="1")          # the 192 x 256 persistent tiles on this small problem
    L = 768
    net = UNetModel(image_size=L, **BIG, dtype=dtype)
    net.load_state_dict({k: torch.from_numpy(gen_param(5, k, tuple(v.shape))) for k, v in net.state_dict().items()})
    ema = EMA(net, decay=0.99)
    ema.load_state_dict({k: torch.from_numpy(gen_param(11, k, tuple(v.shape))) for k, v in net.state_dict().items()})
    x = torch.from_numpy(normal((B, 1, L), seed=3)).cuda(); t = torch.from_numpy(timesteps(B, seed=4)).cuda()
    net.eval()
    flat0 = net.flat.clone(); y_raw = net(x, timesteps=t).clone()
    tape0 = net._tape_id
    with ema.applied() as inside:
        assert inside is net and net._tape_id > tape0
        assert torch.equal(ema.shadow, flat0) and not torch.equal(net.flat, flat0)      # exchanged, not copied
        sd_in = net.state_dict()
        with pytest.raises(RuntimeError, match="nest"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError):
            ema.update()
        y_in = net(x, timesteps=t).clone()
        tape1 = net._tape_id
    assert net._tape_id > tape1
    assert torch.equal(net.flat.view(torch.int32), flat0.view(torch.int32))
    sd_ema = ema.state_dict()
    assert list(sd_in) == list(sd_ema) and all(torch.equal(sd_in[k], sd_ema[k]) for k in sd_ema)
    fresh = UNetModel(image_size=L, **BIG, dtype=dtype)
    fresh.load_state_dict(sd_ema); fresh.eval()
    y_fresh = fresh(x, timesteps=t)
    assert torch.equal(y_in.view(torch.int32), y_fresh.view(torch.int32)), float((y_in - y_fresh).abs().max())
    assert not torch.equal(y_in, y_raw)
    assert torch.equal(net(x, timesteps=t).view(torch.int32), y_raw.view(torch.int32)), "raw weight copies not restored"
    # copy_to: the averaged weights for good
    ema.copy_to(fresh)          # (already there: unchanged)
    assert torch.equal(fresh(x, timesteps=t).view(torch.int32), y_in.view(torch.int32))
    ema.copy_to()
    assert torch.equal(net.flat, ema.shadow) and torch.equal(net(x, timesteps=t).view(torch.int32), y_in.view(torch.int32))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_guided_sampling_under_applied_equals_a_fresh_model(dtype):
    from eegldm.models import UNetModel
    from eegldm.sampling import ddim_sample, make_sampling_scheduler
    from eegldm.training import EMA
    cfg = dict(BIG, image_size=768, num_classes=6)
    net = UNetModel(**cfg, dtype=dtype)
    net.load_state_dict({k: torch.from_numpy(gen_param(5, k, tuple(v.shape))) for k, v in net.state_dict().items()})
    ema = EMA(net)
    ema.load_state_dict({k: torch.from_numpy(gen_param(13, k, tuple(v.shape))) for k, v in net.state_dict().items()})
    sched = make_sampling_scheduler(4)
    nz = torch.from_numpy(normal((3, 1, 768), seed=21)).cuda()
    kw = dict(labels=[4, 0, 2], guidance_scale=3.0, null_class=5, crop=0)
    flat0 = net.flat.clone()
    w_raw, _ = ddim_sample(net, None, sched, nz, **kw)
    with ema.applied():
        w_in, lat_in = ddim_sample(net, None, sched, nz, **kw)
    fresh = UNetModel(**cfg, dtype=dtype)
    fresh.load_state_dict(ema.state_dict())
    w_fresh, lat_fresh = ddim_sample(fresh, None, sched, nz, **kw)
    assert torch.equal(w_in, w_fresh) and torch.equal(lat_in, lat_fresh) and not torch.equal(w_in, w_raw)
    assert torch.equal(net.flat, flat0)
    w_again, _ = ddim_sample(net, None, sched, nz, **kw)
    assert torch.equal(w_again, w_raw)


def test_two_identical_runs_give_identical_shadows(env_switches):
    from eegldm.training import Adam, EMA
    env_switches(EEGLDM_DETERMINISTIC="1")
    shadows = []
    for _ in range(2):
        net, _ = _tiny_unet()
        ema = EMA(net, decay=0.99)
        _train_steps(net, Adam(net, lr=1e-3, ema=ema), 20)
        assert ema.num_updates == 20
        shadows.append((ema.shadow.clone(), net.flat.clone()))
    assert torch.equal(shadows[0][1], shadows[1][1]) and torch.equal(shadows[0][0].view(torch.int32), shadows[1][0].view(torch.int32))
    assert not torch.equal(shadows[0][0], shadows[0][1])


# ---------------------------------------------------------------------------------------------------------------- entry scripts
CK_KEYS = {"epoch", "diffusion", "optimizer", "best_loss", "scale_factor", "scaler", "steps"}


def _ldm_setup(tmp_path, n_recordings, n_samples, n_epochs=6):
    """Synthetic recordings + yaml configs + a stage-1 checkpoint; returns (out dir, common train_ldm arguments, sampler arguments)."""
    import yaml
    from eegldm.models import AutoencoderKL
    from test_gpu_entry import AEKL_YAML, LDM_YAML
    out = str(tmp_path)
    rec = tmp_path / "rec"; rec.mkdir()
    r = np.random.default_rng(0)
    for i in range(n_recordings):
        np.save(rec / f"night{i}.npy", (1e-5 * r.standard_normal((1, n_samples))).astype(np.float64))
    a_yaml, l_yaml = os.path.join(out, "aekl.yaml"), os.path.join(out, "ldm.yaml")
    a = dict(AEKL_YAML); a["train"] = dict(a["train"], output_dir=out)
    l = dict(LDM_YAML); l["train"] = dict(l["train"], output_dir=out, n_epochs=n_epochs)
    yaml.safe_dump(a, open(a_yaml, "w")); yaml.safe_dump(l, open(l_yaml, "w"))
    torch.manual_seed(3)
    ae = AutoencoderKL(**a["autoencoderkl"]["params"])
    run_a = os.path.join(out, "aekl"); os.makedirs(run_a)
    torch.save({k: v.cpu() for k, v in ae.state_dict().items()}, os.path.join(run_a, "best_model.pth"))
    train = ["--config_file", l_yaml, "--autoencoderkl_config_file_path", a_yaml, "--best_model_path", run_a, "--path_pre_processed", str(rec),
             "--latent_channels", "1"]
    sample = ["--output_dir", out, "--best_model_path", run_a, "--autoencoderkl_config_file_path", a_yaml, "--ldm_config_file_path", l_yaml,
              "--start_seed", "3", "--stop_seed", "4", "--num_inference_steps", "4", "--latent_channels", "1"]
    return out, train, sample


def test_train_ldm_with_ema_writes_shadow_and_sampler_uses_it(tmp_path):
    from eegldm.entry import train_ldm as TL, sample_trials as ST
    out, train, sample = _ldm_setup(tmp_path, 4, 15000)
    run = TL.main(TL.parse_args(train + ["--ema_decay", "0.9", "--max_steps", "6"]))
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert set(ck) == CK_KEYS | {"ema"}
    assert set(ck["ema"]) == {"decay", "warmup", "num_updates", "best_loss", "shadow"}
    assert ck["ema"]["num_updates"] == 6 and ck["steps"] == 6 and ck["ema"]["decay"] == 0.9 and ck["ema"]["warmup"] is True
    final, final_ema = torch.load(os.path.join(run, "final_model.pth")), torch.load(os.path.join(run, "final_model_ema.pth"))
    assert list(final_ema) == list(final) == list(ck["ema"]["shadow"])
    assert all(torch.equal(final_ema[k], ck["ema"]["shadow"][k]) for k in final)
    assert all(final_ema[k].shape == final[k].shape for k in final) and any(not torch.equal(final_ema[k], final[k]) for k in final)
    assert all(torch.equal(final[k], ck["diffusion"][k]) for k in final)
    best_ema = torch.load(os.path.join(run, "best_model_ema.pth"))
    assert list(best_ema) == list(final)
    # *_ema.pth is a plain model state dict: it loads into the model as it is
    from eegldm.models import UNetModel
    from test_gpu_entry import LDM_YAML
    up = dict(LDM_YAML["model"]["params"]["unet_config"]["params"], in_channels=1, out_channels=1)
    UNetModel(**up).load_state_dict(final_ema)
    raw_dir = ST.main(ST.parse_args(sample + ["--diffusion_path", run]))
    raw = np.load(os.path.join(raw_dir, "sample_3.npy"))
    ema_dir = ST.main(ST.parse_args(sample + ["--diffusion_path", run, "--use_ema"]))
    avg = np.load(os.path.join(ema_dir, "sample_3.npy"))
    assert raw.shape == avg.shape == (1, 1, 3000) and np.isfinite(raw).all() and np.isfinite(avg).all()
    assert not np.array_equal(raw, avg)


def test_train_ldm_without_ema_is_unchanged_and_use_ema_names_the_missing_file(tmp_path):
    from eegldm.entry import train_ldm as TL, sample_trials as ST
    out, train, sample = _ldm_setup(tmp_path, 4, 15000)
    run = TL.main(TL.parse_args(train + ["--max_steps", "2"]))
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert set(ck) == CK_KEYS
    assert sorted(f for f in os.listdir(run) if f.endswith(".pth")) == ["best_model.pth", "checkpoint.pth", "final_model.pth"]
    with pytest.raises(FileNotFoundError, match="best_model_ema.pth"):
        ST.main(ST.parse_args(sample + ["--diffusion_path", run, "--use_ema"]))
    # resuming that checkpoint with --ema_decay starts the average from the loaded weights
    run2 = TL.main(TL.parse_args(train + ["--max_steps", "1", "--ema_decay", "0.5", "--ema_no_warmup"]))
    ck2 = torch.load(os.path.join(run2, "checkpoint.pth"))
    assert run2 == run and ck2["steps"] == 3 and ck2["ema"]["num_updates"] == 1 and ck2["ema"]["warmup"] is False
    k = "input_blocks.0.0.weight"      # shadow = 0.5 * loaded + 0.5 * updated: strictly between the two checkpoints' weights
    lo, hi = torch.minimum(ck["diffusion"][k], ck2["diffusion"][k]), torch.maximum(ck["diffusion"][k], ck2["diffusion"][k])
    sh = ck2["ema"]["shadow"][k]
    assert bool(((sh >= lo) & (sh <= hi)).all()) and not torch.equal(sh, ck2["diffusion"][k])


def test_train_ldm_ema_resume_is_bit_exact(tmp_path):
    """3 steps + resume + 3 steps == 6 straight steps, shadow and weights, under --deterministic.  One recording of exactly one window:
    the loader's shuffle and crop draws are not part of a checkpoint, so only a data set with a single possible batch gives both runs the
    same batches; everything the EMA adds to the checkpoint is exercised all the same."""
    from eegldm._lib import set_deterministic
    from eegldm.entry import train_ldm as TL
    try:
        (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
        _, train_a, _ = _ldm_setup(tmp_path / "a", 1, 3000)
        _, train_b, _ = _ldm_setup(tmp_path / "b", 1, 3000)
        flags = ["--ema_decay", "0.9", "--deterministic"]
        run_a = TL.main(TL.parse_args(train_a + flags + ["--max_steps", "6"]))
        run_b = TL.main(TL.parse_args(train_b + flags + ["--max_steps", "3"]))
        half = torch.load(os.path.join(run_b, "checkpoint.pth"))
        assert half["ema"]["num_updates"] == 3 and half["steps"] == 3
        assert TL.main(TL.parse_args(train_b + flags + ["--max_steps", "3"])) == run_b
    finally:
        set_deterministic(False)
    a, b = torch.load(os.path.join(run_a, "checkpoint.pth")), torch.load(os.path.join(run_b, "checkpoint.pth"))
    assert a["steps"] == b["steps"] == 6 and a["ema"]["num_updates"] == b["ema"]["num_updates"] == 6
    assert float(a["scale_factor"]) == float(b["scale_factor"])
    for k in a["diffusion"]:
        assert torch.equal(a["diffusion"][k], b["diffusion"][k]), f"raw weights differ after the resume: {k}"
        assert torch.equal(a["ema"]["shadow"][k], b["ema"]["shadow"][k]), f"shadow differs after the resume: {k}"
    fa, fb = torch.load(os.path.join(run_a, "final_model_ema.pth")), torch.load(os.path.join(run_b, "final_model_ema.pth"))
    assert all(torch.equal(fa[k], fb[k]) for k in fa)


def test_train_ldm_scores_the_ema_on_the_validation_split(tmp_path):
    """With a validation split the averaged weights get their own loss (validate under ema.applied()) and their own best file; the raw
    weights are back afterwards (checkpoint == final model)."""
    from eegldm.entry import train_ldm as TL
    out, train, _ = _ldm_setup(tmp_path, 4, 15000, n_epochs=2)
    ids = os.path.join(out, "ids.csv")
    with open(ids, "w") as f:
        f.write("FILE_NAME_EEG\n" + "".join(f"night{i}\n" for i in range(4)))
    run = TL.main(TL.parse_args(train + ["--path_train_ids", ids, "--path_valid_ids", ids, "--ema_decay", "0.9"]))
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert ck["ema"]["num_updates"] == 2 and np.isfinite(ck["ema"]["best_loss"]) and np.isfinite(ck["best_loss"])
    assert ck["ema"]["best_loss"] != ck["best_loss"]
    final = torch.load(os.path.join(run, "final_model.pth"))
    assert all(torch.equal(final[k], ck["diffusion"][k]) for k in final)
    assert os.path.exists(os.path.join(run, "best_model_ema.pth"))


def test_train_dm_with_ema_and_sampler(tmp_path):
    import yaml
    from eegldm.entry import train_dm as TD, sample_trials_dm as SD
    from test_gpu_entry import LDM_YAML
    out = str(tmp_path)
    d_yaml = os.path.join(out, "dm.yaml")
    d = dict(LDM_YAML); d["train"] = dict(d["train"], output_dir=out, run_dir="dm_eeg", batch_size=4, n_epochs=2)
    yaml.safe_dump(d, open(d_yaml, "w"))
    run = TD.main(TD.parse_args(["--config_file", d_yaml, "--synthetic_windows", "4", "--max_steps", "2", "--ema_decay", "0.9"]))
    ck = torch.load(os.path.join(run, "checkpoint.pth"))
    assert set(ck) == {"epoch", "diffusion", "optimizer", "best_loss", "steps", "scaler", "ema"} and ck["ema"]["num_updates"] == 2
    final, final_ema = torch.load(os.path.join(run, "final_model.pth")), torch.load(os.path.join(run, "final_model_ema.pth"))
    assert list(final) == list(final_ema) and all(torch.equal(final_ema[k], ck["ema"]["shadow"][k]) for k in final)
    assert any(not torch.equal(final_ema[k], final[k]) for k in final) and os.path.exists(os.path.join(run, "best_model_ema.pth"))
    args = ["--output_dir", out, "--config_file", d_yaml, "--diffusion_path", run, "--start_seed", "1", "--stop_seed", "2", "--num_inference_steps", "3"]
    raw = np.load(os.path.join(SD.main(SD.parse_args(args)), "sample_1.npy"))
    avg = np.load(os.path.join(SD.main(SD.parse_args(args + ["--use_ema"])), "sample_1.npy"))
    assert avg.shape == (1, 1, 3000) and np.isfinite(avg).all() and not np.array_equal(raw, avg)
