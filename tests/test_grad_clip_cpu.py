"""CPU: the host side of gradient-norm clipping and gradient accumulation -- constructor refusals, the flags of the three training
scripts, the group schedule, the checkpoint entry and its precedence on resume, and the new symbols of the C ABI."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_model(n=8):
    return types.SimpleNamespace(flat=torch.arange(n, dtype=torch.float32), flat_grad=torch.zeros(n), entries={"w": (0, n, (n,))},
                                 sync_weights=lambda: None, ctx=types.SimpleNamespace(sync=lambda: None))


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan")])
def test_constructor_refuses_before_any_device_call(bad):
    from eegldm.training import Adam, clip_grad_norm_
    poison = types.SimpleNamespace()           # touching any attribute of the model (let alone its device) would raise AttributeError
    with pytest.raises(ValueError, match="max_grad_norm"):
        Adam(poison, max_grad_norm=bad)
    with pytest.raises(ValueError, match="max_norm"):
        clip_grad_norm_(poison, bad)


def test_constructor_state():
    from eegldm.training import Adam
    md = _host_model()
    plain, clip, measure = Adam(md), Adam(md, max_grad_norm=0.5), Adam(md, max_grad_norm=float("inf"))
    assert plain.max_grad_norm is None and plain._clip is None
    assert clip.max_grad_norm == 0.5 and measure.max_grad_norm == float("inf")
    assert clip._clip.shape == (8,) and clip._clip.dtype == torch.float32 and float(clip._clip.abs().sum()) == 0.0
    assert clip.clip_stats() == {"last_norm": 0.0, "max_norm_seen": 0.0, "clipped": 0, "steps": 0}
    assert clip.grad_norm.data_ptr() == clip._clip.data_ptr()            # a view of state[0], not a copy
    with pytest.raises(RuntimeError):
        plain.clip_stats()
    # not optimizer state: torch's layout, whatever max_grad_norm is
    assert plain.state_dict().keys() == clip.state_dict().keys() == {"state", "param_groups"}
    assert clip.state_dict()["param_groups"] == plain.state_dict()["param_groups"]
    clip.set_max_grad_norm(None)
    assert clip.max_grad_norm is None and clip._clip is None


def _parsers():
    from eegldm.entry import train_autoencoderkl, train_dm, train_ldm
    return {"ldm": (train_ldm.parse_args, ["--config_file", "c.yaml", "--autoencoderkl_config_file_path", "a.yaml"]),
            "dm": (train_dm.parse_args, ["--config_file", "c.yaml"]),
            "aekl": (train_autoencoderkl.parse_args, ["--config_file", "c.yaml"])}


@pytest.mark.parametrize("script", ["ldm", "dm", "aekl"])
def test_flag_parsing(script, capsys):
    parse, base = _parsers()[script]
    a = parse(base)
    assert a.max_grad_norm is None and getattr(a, "grad_accum_steps", None) is None
    a = parse(base + ["--max_grad_norm", "0.5"])
    assert a.max_grad_norm == 0.5
    assert parse(base + ["--max_grad_norm", "inf"]).max_grad_norm == float("inf")
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            parse(base + ["--max_grad_norm", bad])
    if script == "aekl":                       # BatchNorm statistics are per micro-batch: no accumulation for the GAN step
        with pytest.raises(SystemExit):
            parse(base + ["--grad_accum_steps", "2"])
    else:
        assert parse(base + ["--grad_accum_steps", "3"]).grad_accum_steps == 3
        for bad in ("0", "-2"):
            with pytest.raises(SystemExit):
                parse(base + ["--grad_accum_steps", bad])
    capsys.readouterr()


@pytest.mark.parametrize("K", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 4, 7, 10])
def test_group_schedule(K, n):
    from eegldm.entry.common import accum_plan, accum_schedule
    sch = accum_schedule(n, K)
    assert len(sch) == n
    for i, s in enumerate(sch):
        assert s["zero"] == (i % K == 0)                                  # the gradient is zeroed at the start of a group only
        last = (i % K == K - 1) or i == n - 1
        assert s["sync"] == s["step"] == last                             # one all-reduce and one optimizer step per group
        k = i % K + 1
        assert s["factor"] == (K / k if last else None)                   # a full group: 1; the short last one: K / k
        assert accum_plan(i, n, K) == (s["zero"], last, k)
    assert sum(s["step"] for s in sch) == -(-n // K)
    assert sch[-1]["step"] and sch[-1]["factor"] == K / ((n - 1) % K + 1)
    # every micro-batch counts 1 / K through grad_scale, a step multiplies by factor: each group's weights add up to one
    tot, groups = 0.0, []
    for s in sch:
        tot += 1.0 / K
        if s["step"]:
            groups.append(tot * s["factor"]); tot = 0.0
    assert groups == pytest.approx([1.0] * len(groups))


@pytest.mark.parametrize("K,n,left,want_steps", [(3, 10, 5, [2, 4]), (4, 10, 4, [3]), (4, 10, 1, [0]), (3, 4, 9, [2, 3]), (1, 7, 2, [0, 1])])
def test_group_schedule_with_max_steps(K, n, left, want_steps):
    """--max_steps counts micro-batches: the group it cuts is stepped with what it has."""
    from eegldm.entry.common import accum_schedule
    sch = accum_schedule(n, K, steps_left=left)
    assert len(sch) == min(n, left)
    assert [i for i, s in enumerate(sch) if s["step"]] == want_steps
    assert sch[-1]["step"] and sch[-1]["factor"] == K / ((len(sch) - 1) % K + 1)
    assert [i for i, s in enumerate(sch) if s["zero"]] == list(range(0, len(sch), K))


def test_checkpoint_entry_only_with_a_flag():
    from eegldm.entry.common import grad_clip_entry
    ns = types.SimpleNamespace
    assert grad_clip_entry(ns(max_grad_norm=None, grad_accum_steps=None)) is None
    assert grad_clip_entry(ns()) is None
    assert grad_clip_entry(ns(max_grad_norm=0.5, grad_accum_steps=None)) == {"max_grad_norm": 0.5, "grad_accum_steps": 1}
    assert grad_clip_entry(ns(max_grad_norm=None, grad_accum_steps=2)) == {"max_grad_norm": None, "grad_accum_steps": 2}
    assert grad_clip_entry(ns(max_grad_norm=1.0)) == {"max_grad_norm": 1.0, "grad_accum_steps": 1}      # train_autoencoderkl has no accumulation flag


def test_resume_precedence(capsys):
    from eegldm.entry.common import grad_clip_resume
    ns = types.SimpleNamespace
    saved = {"grad_clip": {"max_grad_norm": 0.5, "grad_accum_steps": 2}}
    a = ns(max_grad_norm=None, grad_accum_steps=None)
    grad_clip_resume(a, saved)                                            # no flags: the checkpoint's values come back
    assert (a.max_grad_norm, a.grad_accum_steps) == (0.5, 2) and capsys.readouterr().out == ""
    a = ns(max_grad_norm=0.5, grad_accum_steps=2)
    grad_clip_resume(a, saved)                                            # the same values: nothing to say
    assert (a.max_grad_norm, a.grad_accum_steps) == (0.5, 2) and capsys.readouterr().out == ""
    a = ns(max_grad_norm=2.0, grad_accum_steps=None)
    grad_clip_resume(a, saved)                                            # the command line wins and says so, in one line
    out = capsys.readouterr().out
    assert (a.max_grad_norm, a.grad_accum_steps) == (2.0, 2)
    assert out.count("\n") == 1 and "max_grad_norm 0.5 -> 2.0" in out
    grad_clip_resume(ns(max_grad_norm=2.0, grad_accum_steps=4), saved, rank=1)
    assert capsys.readouterr().out == ""                                  # rank 0 prints
    a = ns(max_grad_norm=None, grad_accum_steps=None)
    grad_clip_resume(a, {})                                               # a checkpoint written without the flags
    assert (a.max_grad_norm, a.grad_accum_steps) == (None, None)
    a = ns(max_grad_norm=None)                                            # train_autoencoderkl: no accumulation flag to restore
    grad_clip_resume(a, saved)
    assert a.max_grad_norm == 0.5 and not hasattr(a, "grad_accum_steps")


def test_new_symbols_in_header_and_binding():
    from eegldm._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "eegldm.h")).read()
    for name, nargs in (("eegldm_grad_norm", 6), ("eegldm_adam_step_clip", 15), ("eegldm_grad_scale_by", 4)):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in include/eegldm.h"
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs
        assert len(SIGNATURES[name]) == nargs
        assert hasattr(lib, name), f"libeegldm.so does not export {name}"
    assert re.search(r"#define EEGLDM_ABI_VERSION 8\b", header)
