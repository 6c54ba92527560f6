"""CPU suite: the base / anab model configurations (scripts/config/kitti_3d_base.py, kitti_3d_anab.py) and every other flag
combination the reference model file accepts (M3d_inference_align.py:138-168): module construction, the state_dict contract,
the composed oracle (tests/config_oracle.py) against the reference's own outputs (tests/golden/model_{base,anab}_128x320_b2.npz,
tools/gen_golden_configs.py)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import config_oracle
from m3dssd_amd import synth
from m3dssd_amd.config import CONFIG_FLAGS, Config, model_flags
from oracle import detect as odet
from tools import gen_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [dict(shape_align=sa, center_align=ca, attention=at)
          for sa, ca, at in itertools.product((False, True), (False, True), ("ANAB", None))]


def _golden(golden_dir, config):
    return np.load(os.path.join(golden_dir, "model_%s_128x320_b2.npz" % config))


def _build(flags, device="cpu"):
    from model.M3d_inference_align import build
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device=device, **flags)
    return conf, build(conf, "test")


def test_named_configs_carry_the_reference_flags():
    assert model_flags(Config()) == (True, True, True)
    assert model_flags(Config("anab_fullalign")) == (True, True, True)
    assert model_flags(Config("anab")) == (False, False, True)
    assert model_flags(Config("base")) == (False, False, False)
    assert Config("base").attention is None
    # any attention other than "ANAB" is "no attention block" (M3d_inference_align.py:168,271)
    conf = Config()
    conf.attention = "PAM"
    assert model_flags(conf) == (True, True, False)
    with pytest.raises(ValueError):
        Config("dla102")


def test_default_synth_recipe_unchanged():
    assert list(synth.param_spec()) == list(synth.param_spec(**CONFIG_FLAGS["anab_fullalign"]))
    assert len(synth.param_spec()) == 542
    full = synth.synth_state_dict(0)
    for config, n in (("base", 526), ("anab", 535)):
        sd = synth.synth_state_dict(0, **synth.config_flags(config))
        assert len(sd) == n
        assert list(sd) == [k for k in full if k in sd]
        for k, v in sd.items():
            assert torch.equal(v, full[k]), k


@pytest.mark.parametrize("flags", COMBOS, ids=lambda f: "sa%d-ca%d-%s" % (f["shape_align"], f["center_align"], f["attention"]))
def test_every_flag_combination_builds_and_loads(flags):
    conf, net = _build(flags)
    sa, ca, anab = model_flags(conf)
    assert (net.shape_align is None) == (not sa)
    assert (net.center_align2d is None) == (not ca) and (net.center_align3d is None) == (not ca)
    assert hasattr(net, "bbox_z3d_gl") == anab
    spec = synth.param_spec(**flags)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(k, tuple(s)) for k, s in spec.items()]
    sd = synth.synth_state_dict(0, **flags)
    net.load_state_dict(sd, strict=True)
    net.load_state_dict({"module." + k: v for k, v in sd.items()}, strict=True)
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # a checkpoint of another configuration is refused, as by the reference's strict load
    other = dict(flags, center_align=not flags["center_align"])
    with pytest.raises(RuntimeError):
        net.load_state_dict(synth.synth_state_dict(0, **other), strict=True)
    net.compute_dtype = "bf16"
    net.reuse_outputs = True
    net.refresh_engine()
    with pytest.raises(NotImplementedError):          # the engine runs on a ROCm device only
        net(torch.zeros(2, 3, 128, 320))


@pytest.mark.parametrize("config,n", [("base", 526), ("anab", 535)])
def test_state_dict_matches_reference_key_list(golden_dir, config, n):
    g = _golden(golden_dir, config)
    _, net = _build(synth.config_flags(config))
    keys = [(k, ",".join(str(d) for d in v.shape)) for k, v in net.state_dict().items()]
    assert len(keys) == n
    assert keys == list(zip(g["keys"].tolist(), g["key_shapes"].tolist()))


def _close(a, b, tol):
    return np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() <= tol


@pytest.mark.parametrize("config", ["base", "anab"])
def test_composed_oracle_matches_reference(golden_dir, config):
    """Bounds of tests/test_oracle_golden.py::test_model_small_matches_reference (fullalign)."""
    g = _golden(golden_dir, config)
    flags = synth.config_flags(config)
    conf = synth.synth_conf((128, 320), 0, batch_size=2, device="cpu", **flags)
    sd = synth.synth_state_dict(0, **flags)
    x = synth.synth_frames(2, (128, 320), 1234)
    taps = {}
    with torch.no_grad():
        cls, prob, b2, b3, fs, rois = config_oracle.rpn_forward(sd, conf, x, taps)
    rs = int(g["row_stride"])
    for name, t in (("cls", cls), ("prob", prob), ("bbox_2d", b2), ("bbox_3d", b3)):
        assert _close(t[:, ::rs].numpy(), g[name], 2e-4), name
        chk = g["chk." + name]
        assert abs(t.double().abs().sum().item() - chk[1]) <= 1e-5 * chk[1] and t.numel() == chk[2]
    chk = g["chk.rois"]
    assert abs(rois.double().sum().item() - chk[0]) <= 1e-9 * abs(chk[1]) and rois.numel() == chk[2]
    assert np.array_equal(fs.numpy(), g["feat_size"])
    taps_seen = [k[4:] for k in g.files if k.startswith("tap.")]
    assert taps_seen == (["feats0", "feats_gl"] if config == "anab" else ["feats0"])
    for name in taps_seen:
        assert _close(taps[name][:, ::8].numpy(), g["tap." + name], 2e-4), name
    # the stages the configuration does not have are identities of the map that stands in for them
    assert taps["feats"] is taps["feats0"] and taps["feats_align3d"] is taps["feats0"]
    if config == "base":
        assert taps["feats_gl"] is taps["feats0"]
    # detection of image 0 against the reference's im_detect_3d (bounds of test_detect_matches_reference_im_detect_3d)
    ab, _, _ = odet.detect_image(prob[0], b2[0], b3[0], rois, conf)
    ref = g["aboxes"]
    assert ab.shape == ref.shape and ref.shape[0] > 0
    assert np.array_equal(ab[:, 13], ref[:, 13]) and np.array_equal(ab[:, 5], ref[:, 5])
    assert np.abs(ab - ref).max() < 1e-3 * max(1.0, np.abs(ref).max())


def test_fullalign_composition_is_the_oracle():
    """With every flag on the composed oracle is oracle.model_cpu.rpn_forward, bit for bit."""
    from oracle import model_cpu
    conf = synth.synth_conf((64, 160), 0, batch_size=1, device="cpu")
    sd = synth.synth_state_dict(0)
    x = synth.synth_frames(1, (64, 160), 1234)
    with torch.no_grad():
        a = config_oracle.rpn_forward(sd, conf, x)
        b = model_cpu.rpn_forward(sd, conf, x)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.skipif(not os.path.isdir(os.path.join(gen_golden.REF, "model")), reason="needs the reference tree (build container only)")
def test_goldens_regenerate_bit_for_bit(golden_dir, tmp_path):
    # a subprocess: the generator's stubs replace modules in sys.modules
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_golden_configs.py"), str(tmp_path)],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for config in ("base", "anab"):
        a, b = _golden(golden_dir, config), _golden(str(tmp_path), config)
        assert a.files == b.files
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (config, k)
