"""GPU tests (-m gpu) of the training augmentation kernel (m3dssd_amd/csrc/augment.hip, m3d_augment_u8) and its host module
(m3dssd_amd/host/augment.py): the identity anchor against the existing preprocess kernel, parity with the float64 restatement of
tests/augment_ref.py on explicit parameters, the golden of the reference's own Augmentation, full-range inputs, host / device
frames, the library's argument checks, and one training iteration fed by TrainAugmentation.

Bound of every parity check: 4x the float32-against-float64 gap of the RESTATEMENT on the same cases (tests/augment_cases.py;
measured 2.3e-6 on the parity cases, 2.2e-6 on the golden, in normalised units).  It never comes from the kernel's output."""
import ctypes

import numpy as np
import pytest
import torch

from gpu_common import _dev, _log
from m3dssd_amd import _hip, synth
from m3dssd_amd.host import augment as A
from m3dssd_amd.host import loss as hl
from m3dssd_amd.host import ops
from m3dssd_amd.host.preprocess import preprocess

import augment_cases as AC
import augment_ref as AR
import rpn_loss_ref as RR

pytestmark = pytest.mark.gpu


def _run(buf, params, size, device=True):
    t = torch.from_numpy(np.ascontiguousarray(buf))
    out = A.augment_batch(t.to(_dev()) if device else t, params, size, AR.MEAN, AR.STDS)
    torch.cuda.synchronize()
    assert out.shape == (len(params), 3, size[0], size[1]) and out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------ identity anchor
@pytest.mark.parametrize("src,size", [((16, 40), (16, 40)), ((16, 38), (16, 38)), ((13, 37), (16, 38)), ((13, 37), (16, 40))])
def test_with_every_probability_zero_it_is_the_preprocess_kernel_bit_for_bit(src, size):
    rng = np.random.RandomState(17)
    frames = rng.randint(0, 256, size=(2,) + src + (3,)).astype(np.uint8)
    conf = AR.AttrDict(distort_prob=0.0, mirror_prob=0.0, trans_prob=0.0, shift=0.1, scale_trans=0.4)
    params = A.draw_params(conf, [src, src], np.random.RandomState(0))
    assert all(p["mode"] == 0 and not p["mirror"] and not p["warped"] for p in params)
    got = _run(frames, params, size)
    want = preprocess(torch.from_numpy(frames).to(_dev()), size, AR.MEAN, AR.STDS).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if src != size:                                                      # the padding is there, and it is the normalised zero
        zero = AC.border_value()
        assert (got[:, :, src[0]:, :] == zero[None, :, None, None]).all() and (got[:, :, :, src[1]:] == zero[None, :, None, None]).all()


# ------------------------------------------------------------------------------------ parity with the float64 restatement
@pytest.mark.parametrize("photo,mirror_first,dest", AC.PARITY_IDS)
def test_parity_with_the_float64_restatement(photo, mirror_first, dest):
    buf, params, r32, r64, masks = AC.parity_case(photo, mirror_first, dest)
    bound = 4 * AC.parity_gap()
    got = _run(buf, params, dest)
    err = float(np.abs(got - r64).max())
    print("augment parity", photo, mirror_first, dest, "max err %.3e bound %.3e, bit-equal to the float32 restatement: %s"
          % (err, bound, np.array_equal(got, r32)))
    _log("augment_parity", dict(photo=photo, mirror_first=mirror_first, dest=list(dest), err=err, bound=bound))
    assert err <= bound
    # the in / out decision of every tap: the border pixels are exactly the restatement's, bit for bit
    zero = AC.border_value()
    for c in range(3):
        assert ((got[:, c] == zero[c]) == masks).all()


@pytest.mark.parametrize("dest", [(37, 520), (37, 518)])
def test_parity_over_more_than_one_block_and_more_than_one_launch(dest):
    """18 images (a launch carries 16) of 50x290 into a destination several blocks wide and high, with and without a row tail."""
    rng = np.random.RandomState(23)
    B, h, w = 18, 50, 290
    buf = rng.randint(40, 216, size=(B, h, w, 3)).astype(np.uint8)
    params = [A.make_params(h - (i % 3), w - (i % 5), mode=i % 3, delta=(-1) ** i * 3.0 * (i % 11), alpha=0.5 + (i % 9) / 8.0,
                            sat=0.5 + (i % 7) / 6.0, hue=(i % 13) * 3.0 - 18.0, mirror=bool(i & 1), warped=True,
                            scale=0.6 + 0.8 * (i % 6) / 5.0, centre=(w * (0.3 + 0.4 * (i % 4) / 3.0), h * (0.3 + 0.4 * (i % 5) / 4.0)))
              for i in range(B)]
    r32 = AR.augment_frames(buf, params, dest, dtype=np.float32)
    r64 = AR.augment_frames(buf, params, dest, dtype=np.float64)
    bound = 4 * float(np.abs(r32 - r64).max())
    got = _run(buf, params, dest)
    err = float(np.abs(got - r64).max())
    print("augment parity", dest, "max err %.3e bound %.3e" % (err, bound))
    assert err <= bound


# ------------------------------------------------------------------------------------ the golden of the reference's Augmentation
@pytest.mark.parametrize("case", AR.golden_cases(), ids=lambda c: c[0])
def test_the_golden_images_from_the_seed(case):
    name, conf, seed, frames, imobjs, size, images, want, scale_factors = case
    bound = 4 * AC.golden_gap()
    aug = A.TrainAugmentation(AR.AttrDict(conf, device="cuda:0"))
    x, imobjs_aug = aug(torch.from_numpy(AR.pack_frames(frames)), imobjs, rng=np.random.RandomState(seed),
                        frame_sizes=[f.shape[:2] for f in frames])
    err = float(np.abs(x.cpu().numpy().astype(np.float64) - images).max())
    print("augment golden on the device", name, "max err %.3e bound %.3e" % (err, bound))
    assert err <= bound
    for i, o in enumerate(imobjs_aug):
        got = AR.label_fields(o)
        for k in AR.GT_FIELDS:
            assert got[k].tobytes() == np.ascontiguousarray(want[i][k], dtype=np.float64).tobytes()


# ------------------------------------------------------------------------------------ full range, determinism, host frames
def _extreme():
    rng = np.random.RandomState(29)
    frames = [rng.choice([0, 255], size=(h, w, 3)).astype(np.uint8) for h, w in AC.SOURCES]
    params = [A.make_params(13, 37, mode=1, delta=-32.0, alpha=1.5, sat=1.5, hue=-18.0, mirror=True, warped=True, scale=0.6, centre=(37 * 0.7, 13 * 0.3)),
              A.make_params(20, 36, mode=2, delta=32.0, alpha=0.5, sat=0.5, hue=18.0, warped=True, scale=1.4, centre=(36 * 0.3, 20 * 0.7)),
              A.make_params(16, 38, mode=2, delta=-32.0, alpha=1.5, sat=1.5, hue=18.0, mirror=True)]
    return AR.pack_frames(frames), params


def test_full_range_inputs_stay_finite_and_two_runs_are_bit_equal():
    buf, params = _extreme()
    for dest in AC.DESTS:
        a, b = _run(buf, params, dest), _run(buf, params, dest)
        assert np.isfinite(a).all()
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_host_and_device_frames_give_the_same_bits():
    buf, params = _extreme()
    a, b = _run(buf, params, (16, 40), device=True), _run(buf, params, (16, 40), device=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pinned = torch.from_numpy(buf).pin_memory()
    c = A.augment_batch(pinned, params, (16, 40), AR.MEAN, AR.STDS, device="cuda:0").cpu().numpy()
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ------------------------------------------------------------------------------------ the library's argument checks
def test_bad_arguments_return_an_error_and_launch_nothing():
    dev = _dev()
    frames = torch.zeros(2, 13, 37, 3, dtype=torch.uint8, device=dev)
    out = torch.full((2, 3, 16, 38), 7.0, device=dev)
    good = A.pack_params([A.make_params(13, 37), A.make_params(13, 37)])
    m3, s3 = (ctypes.c_float * 3)(*AR.MEAN), (ctypes.c_float * 3)(*AR.STDS)
    L = _hip.lib()

    def call(N, rows):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.m3d_augment_u8(frames.data_ptr(), N, 13, 37, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), A.PARAM_COLS, m3, s3,
                              out.data_ptr(), 16, 38, st)
        torch.cuda.synchronize()
        return rc

    oversized, singular = good.copy(), good.copy()
    oversized[1, 0] = 14                                 # the SECOND image: the first must not have been launched either
    singular[1, 8] = 0.0
    for N, rows in ((2, oversized), (0, good), (2, singular)):
        assert call(N, rows) != 0
        assert L.m3d_last_error().decode().startswith("augment_u8")
        assert (out == 7.0).all()
    assert call(2, good) == 0 and not (out == 7.0).any()


# ------------------------------------------------------------------------------------ end to end
def test_one_training_iteration_from_uint8_frames():
    from lib.loss.rpn_3d import RPN_3D_loss
    from model.M3d_inference_align import build
    dev = _dev()
    crop, B = (128, 320), 2
    flags = synth.config_flags("base")
    conf = RR.loss_conf(crop, 0, device="cuda:0")
    conf.update(flags)
    conf.batch_size = B
    conf.update(mirror_prob=0.5, trans_prob=0.7, shift=0.1, scale_trans=0.4, distort_prob=-1)
    net = build(conf, "train")
    net.load_state_dict(synth.synth_state_dict(0, **flags), strict=True)
    net = net.to(dev).train()
    rng = np.random.RandomState(41)
    frames = torch.from_numpy(rng.randint(0, 256, size=(B, 120, 310, 3)).astype(np.uint8))
    imobjs = AC.train_imobjs(43, (120, 310), B)
    aug = A.TrainAugmentation(conf)
    x, imobjs_aug = aug(frames, imobjs, rng=np.random.RandomState(3))
    params = A.draw_params(conf, [(120, 310)] * B, np.random.RandomState(3))
    assert any(p["warped"] for p in params) and any(p["mirror"] for p in params)
    assert x.shape == (B, 3) + crop and x.is_cuda and torch.isfinite(x).all()
    # the labels that travel on are the host transform's, and so are the targets computed from them
    host = [A.transform_labels(o, p) for o, p in zip(imobjs, params)]
    table, table_host = (hl.pack_gts(o, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h) for o in (imobjs_aug, host))
    assert np.array_equal(table, table_host) and not np.array_equal(table, hl.pack_gts(imobjs, conf.lbls, conf.ilbls, conf.min_gt_vis, conf.min_gt_h))
    crit = RPN_3D_loss(conf)
    cls, prob, b2, b3, fs = net(x)
    fs = [int(v) for v in fs]
    tg = [ops.rpn_precompute_targets(np.asarray(conf.anchors, dtype=np.float64), crit._conf_vec(), t, fs, dev) for t in (table, table_host)]
    for k in ("labels", "gt_index", "bbox_2d", "bbox_3d"):
        assert torch.equal(tg[0][k], tg[1][k])
    assert (tg[0]["labels"] > 0).any()
    loss, stats = crit(cls, prob, b2, b3, imobjs_aug, fs)
    assert torch.isfinite(loss)
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(torch.isfinite(g).all() for g in grads)
    assert any(g.abs().max().item() > 0 for g in grads)
