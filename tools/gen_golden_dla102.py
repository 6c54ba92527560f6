#!/usr/bin/env python
"""Generate tests/golden/model_dla102_{anab_fullalign,base}_128x320_b2.npz by running the REFERENCE's own model file with the
backbone the shipped configurations use (scripts/config/kitti_3d_*.py: ``conf.back_bone = 'dla102'``).

Build-container only, like tools/gen_golden_configs.py (whose layout it writes and whose stubs, from tools/gen_golden.py, it
reuses): needs the reference tree and never travels to the GPU box.  Per configuration it builds
``model.M3d_inference_align.build(conf, 'test')`` with ``back_bone='dla102'`` and ``pre_train=None`` -- the reference's dla102()
tests ``pretrained is not None``, so False would reach load_pretrained_model -> model_zoo.load_url, a download --, loads the seed-0
synthetic DLA-102 state_dict with strict=True (the key list of the reference's own module must equal
``synth.param_spec(back_bone='dla102')`` in order), runs B=2 frames of 128x320 and writes ``cls`` / ``prob`` / ``bbox_2d`` /
``bbox_3d`` every ``row_stride``-th row, ``tap.feats0`` (``tap.feats_gl`` with ANAB) on every 16th channel, ``chk.*`` checksums,
``keys`` / ``key_shapes`` and the ``aboxes`` rows of the reference's im_detect_3d on image 0.

Run:  python tools/gen_golden_dla102.py [OUT_DIR]       (default tests/golden; about a minute)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden  # noqa: E402

CONFIGS = ("anab_fullalign", "base")
CROP, BATCH, ROW_STRIDE, TAP_STRIDE = (128, 320), 2, 4, 16
TAPS = {"base": "feats0", "bbox_z3d_gl": "feats_gl"}


def golden_name(config):
    return "model_dla102_%s_%dx%d_b%d.npz" % (config, CROP[0], CROP[1], BATCH)


def main(out_dir):
    gen_golden._install_stubs()
    import torch
    torch.set_num_threads(8)
    from m3dssd_amd import synth
    import lib.rpn_util as ref_rpn
    import model.M3d_inference_align as ref_model
    from easydict import EasyDict

    os.makedirs(out_dir, exist_ok=True)
    checks = gen_golden._checks
    for config in CONFIGS:
        flags = synth.config_flags(config)
        conf = synth.synth_conf(CROP, 0, batch_size=BATCH, device="cpu", back_bone="dla102", **flags)
        conf.pre_train = None
        sd = synth.synth_state_dict(0, back_bone="dla102", **flags)
        net = ref_model.build(EasyDict(dict(conf)), "test")
        net.load_state_dict(sd, strict=True)
        ref_keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert ref_keys == [(k, tuple(v.shape)) for k, v in sd.items()], "state_dict contract mismatch (%s)" % config
        x = synth.synth_frames(BATCH, CROP, 1234)
        taps, hooks = {}, []
        mods = dict(net.named_modules())
        for mname, tname in TAPS.items():
            if mname in mods:
                hooks.append(mods[mname].register_forward_hook(
                    lambda m, i, o, tname=tname: taps.__setitem__(tname, o.detach().clone())))
        with torch.no_grad():
            out = net(x)
        for h in hooks:
            h.remove()
        cls, prob, b2, b3, fs, rois = out
        rs = ROW_STRIDE
        g = {"row_stride": np.array(rs), "tap_stride": np.array(TAP_STRIDE), "cls": cls[:, ::rs].numpy(),
             "prob": prob[:, ::rs].numpy(), "bbox_2d": b2[:, ::rs].numpy(), "bbox_3d": b3[:, ::rs].numpy(),
             "feat_size": fs.numpy()}
        for name, t in (("cls", cls), ("prob", prob), ("bbox_2d", b2), ("bbox_3d", b3), ("rois", rois)):
            g["chk." + name] = checks(t)
        for k, v in taps.items():
            g["tap." + k] = v[:, ::TAP_STRIDE].numpy()
            g["chk." + k] = checks(v)
        g["keys"] = np.array([k for k, _ in ref_keys])
        g["key_shapes"] = np.array([",".join(str(d) for d in s) for _, s in ref_keys])

        # im_detect_3d on the reference outputs (image 0), .cuda() shimmed away
        cuda, float_tensor = torch.Tensor.cuda, getattr(torch.cuda, "FloatTensor", None)
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.cuda.FloatTensor = torch.FloatTensor

        class Obj:
            imH, imW, p2, scale_factor = CROP[0], CROP[1], np.eye(4), 1.0

        class FakeNet:
            def eval(self):
                return self

            def __call__(self, im):
                return tuple(o.clone() for o in out)
        try:
            g["aboxes"] = ref_rpn.im_detect_3d(x[:1], FakeNet(), EasyDict(dict(conf)), Obj())
        finally:
            torch.Tensor.cuda = cuda
            torch.cuda.FloatTensor = float_tensor
        path = os.path.join(out_dir, golden_name(config))
        np.savez_compressed(path, **g)
        fg = (1 - prob[:, :, 0]).view(BATCH, -1, CROP[0] // 8, CROP[1] // 8).max(dim=1)[0]
        print("%-14s %d keys, hard-mask fraction %.3f, %d detections, %s %.1f KB"
              % (config, len(ref_keys), (fg > 0.5).float().mean().item(), g["aboxes"].shape[0], path,
                 os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else gen_golden.OUT)
