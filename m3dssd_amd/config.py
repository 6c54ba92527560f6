"""Configuration object for the M3DSSD inference path.

The reference passes an ``EasyDict`` (scripts/config/kitti_3d_anab_fullalign.py:4-152,
re-read from a pickle at test time, scripts/test_rpn_3d.py:27).  ``Conf`` gives the
same access patterns (attribute, ``in``, ``[]``) without the easydict dependency;
``Config()`` fills the fields RPN/DLASeg read (M3d_inference_align.py:41-63,138-168,
pose_dla_dcn.py:529) with the shipped values, except ``back_bone`` which defaults to
``dla34`` (BASELINE.json north_star); the shipped configurations' ``dla102`` is
``Config(back_bone="dla102")`` (fp32 only, see BACK_BONES).

The reference ships three configurations of the one model file; they differ in the three
flags of ``CONFIG_FLAGS`` (scripts/config/kitti_3d_base.py, kitti_3d_anab.py,
kitti_3d_anab_fullalign.py: lines 14-18).  ``Config()`` is the fullalign one;
``Config("base")`` / ``Config("anab")`` give the other two.
"""
import numpy as np


class Conf(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def copy(self):
        return Conf(dict.copy(self))


BACK_BONES = ("dla34", "dla102")

CONFIG_FLAGS = {
    "base": dict(attention=None, center_align=False, shape_align=False),
    "anab": dict(attention="ANAB", center_align=False, shape_align=False),
    "anab_fullalign": dict(attention="ANAB", center_align=True, shape_align=True),
}


def model_flags(conf):
    """(shape_align, center_align, anab) of a conf, read the way RPN.__init__ / forward of the reference read them
    (M3d_inference_align.py:138-168,241-277): any ``attention`` other than "ANAB" means no attention block."""
    attention = conf["attention"] if "attention" in conf else None
    return bool(conf["shape_align"]), bool(conf["center_align"]), attention == "ANAB"


def Config(name="anab_fullalign", back_bone="dla34"):
    if name not in CONFIG_FLAGS:
        raise ValueError("unknown configuration %r (one of %s)" % (name, ", ".join(sorted(CONFIG_FLAGS))))
    if back_bone not in BACK_BONES:
        raise ValueError("unknown back_bone %r (one of %s)" % (back_bone, ", ".join(BACK_BONES)))
    conf = Conf()
    conf.model = "M3d_inference_align"
    conf.ida_dcnv2 = True
    conf.update(CONFIG_FLAGS[name])
    conf.image_means = [0.485, 0.456, 0.406]
    conf.image_stds = [0.229, 0.224, 0.225]
    conf.feat_stride = 8
    conf.back_bone = back_bone
    conf.pre_train = False
    conf.test_scale = [384, 1280]
    conf.crop_size = [384, 1280]
    conf.percent_anc_h = [0.0625, 0.75]
    conf.min_gt_h = conf.test_scale[0] * conf.percent_anc_h[0]
    conf.max_gt_h = conf.test_scale[0] * conf.percent_anc_h[1]
    conf.lbls = ["Car", "Pedestrian", "Cyclist"]
    conf.ilbls = ["Van", "ignore"]
    conf.batch_size = 4
    conf.nms_topN_pre = 3000
    conf.nms_topN_post = 40
    conf.nms_thres = 0.4
    conf.clip_boxes = False
    conf.cluster_anchors = 0
    conf.anchors = None
    conf.bbox_means = None
    conf.bbox_stds = None
    base = (conf.max_gt_h / conf.min_gt_h) ** (1 / (12 - 1))
    conf.anchor_scales = np.array([conf.min_gt_h * (base ** i) for i in range(0, 12)])
    conf.anchor_ratios = np.array([0.5, 1.0, 1.5])
    conf.device = "cuda:0"
    return conf
