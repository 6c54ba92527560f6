"""Throughput mode: a software-pipelined detector (``PipelinedDetector``); single-frame mode: ``FrameDetector`` (at the end).

The post-forward stage (64-bit-key top-k, decode, NMS, row selection -- lib/rpn_util.py:1442-1555 in the reference)
is latency-bound and leaves the chip mostly idle for ~0.35 ms per batch.  ``PipelinedDetector`` overlaps it with
the forward of the NEXT batch: one captured hipGraph per input shape whose two branches are

    branch A (main stream):  forward(batch k)  [the launches in front of the first head that writes the planar staging]
    branch B (side stream):  detect(batch k-1) on the planar head outputs + sort keys the previous replay left
    join, then the heads of batch k and ``m3d_score_keys_planar`` -> what branch B of the next replay will read

so each ``step(x)`` returns the detections of the PREVIOUS batch (one batch of pipeline latency) and ``flush()``
drains the last one.  Results are identical to ``lib.rpn_util.detect_batch`` (tests/test_gpu_detect.py).

The detection stage needs 3000 decoded rows per image, not the bundled ``cls / prob / bbox_2d / bbox_3d`` tensors
(M3d_inference_align.py:280-301: 38 MB per image written and read back, 2.5 GB per step at bs = 64): ``planar=True`` (default)
replaces ``m3d_bundle_outputs`` by the key-only pass and decodes from the planar staging (``m3d_topk_decode_planar``, same
bits); ``planar=False`` (or M3D_PIPE_PLANAR=0) is the bundled form: detect(k-1) beside forward(k), join, bundle(k).  In the
planar form ``plan.named["prob" / "bbox_2d" / "bbox_3d" / "cls"]`` are NOT written by a replay.

``defer_3d`` (default: on whenever the sparse heads are on and the plan offers ``post3d``; ``M3D_DEFER_3D=0`` or ``False``: off) moves
what only the surviving boxes need out of the forward: the heads behind columns 8..12 of a row (z3d, w3d, h3d, l3d, rY3d) and the ANAB
attention run on branch B, behind the NMS and ``m3d_select_post``, at the pixels of the at most ``nms_topN_post`` rows per image that
were selected (``m3d_topk_decode_planar_2d`` -> NMS -> ``m3d_select_post`` -> ``m3d_post_rows`` -> ``plan.post3d`` ->
``m3d_fill_post_3d``); the forward behind the join runs ``plan.tail_pre``.  Same bits (tests/test_gpu_post_nms_heads.py).

``u8_frame=(h, w)`` is the fed-input form (the reference pays ``im.cuda()`` per frame, lib/rpn_util.py:1427-1429,
and preprocesses on the host, lib/dataloader.py:934-950, lib/augmentations.py:472-501): raw uint8 BGR frames [B, h, w, 3] sit in
PINNED host memory; the graph of batch k carries, on its side branch, an upload KERNEL (``m3d_upload_indirect``) that streams
the frames of batch k + 1 over PCIe into the second of TWO device buffers while the forward of batch k runs on the first, and the
stem reads uint8 frames directly (``m3d_stem_conv7x7_u8``: padding to the crop size, /255, -mean, /stds, BGR->RGB in its loads).
Two graphs are captured, one per input buffer; which host buffer a replay uploads is named by an 8-byte word in pinned host
memory that the host writes before the replay (no copy engine, no copy stream, no events: a hipMemcpyAsync next to the graph
cost more step time than a serial copy on this platform, tools/feed_probe.py).

``refine=True`` appends the post-NMS 3-D refinement of ``test_kitti_3d`` (lib/rpn_util.py:1796-1847: back to the original image
scale, clipping, alpha -> ry, hill climbing, back-projection; ``m3d_refine_3d_ex``) to branch B, reading the selected rows where
``m3d_select_post`` left them: a replay then yields the rows of the KITTI result files of batch k-1.
"""
import ctypes
import math
import os

import torch

from . import _hip
from .host.detect import (detect_from_outputs, detect_from_planar, detect_from_planar_2d, detect_from_planar_mw, fill_post_3d,
                          post_rows, score_keys_planar, select_block, unwrap)
from .host.refine import RefineMeta, refine_rows


class _Detector:
    """What both detectors own: the module, its engine and plan, the input buffers, the refinement's buffers, and the pieces of a
    captured step -- plan ops with the input pointer set, rows -> selection -> optional refinement, the result tuple."""

    def __init__(self, net, conf, batch, height, width, refine, score_thresh, step_r_init, r_lim, u8_frame, u8_buffers,
                 sparse_heads=None, planar=True):
        net = unwrap(net)                               # (a DataParallel / DDP wrapper of the module, as the reference's scripts pass it)
        self.net, self.conf = net, conf
        dev = next(net.parameters()).device
        if dev.type != "cuda":
            raise NotImplementedError("%s needs the module on a ROCm device" % type(self).__name__)
        self.dev = dev
        self.batch = int(batch)
        self.refine = bool(refine)
        self.u8_frame = None if u8_frame is None else (int(u8_frame[0]), int(u8_frame[1]))
        self._rargs = (float(score_thresh), bool(getattr(conf, "hill_climbing", True)), float(step_r_init), float(r_lim))
        self.eng = net.engine()
        self.plan = self.eng.plan_for(self.batch, height, width)
        if self.u8_frame is None:
            self.input = torch.zeros(self.batch, 3, height, width, device=dev, dtype=torch.float32)
        else:
            fh, fw = self.u8_frame
            if fh > height or fw > width:
                raise RuntimeError("u8_frame %dx%d does not fit the padded size %dx%d" % (fh, fw, height, width))
            nbytes = self.batch * fh * fw * 3
            self._u8_bytes = nbytes
            self._u8_flat = [torch.zeros(-(-nbytes // 16) * 16, device=dev, dtype=torch.uint8) for _ in range(u8_buffers)]
            self.inputs_u8 = [t[:nbytes].view(self.batch, fh, fw, 3) for t in self._u8_flat]
            self.input = self.inputs_u8[0]
        assert self.plan.ops[-1][0] == "bundle_outputs"
        self.n_fwd = len(self.plan.ops) - 1                 # planar form: everything in front of the output bundling
        # box heads at the needed pixels only (the plan's detection-only tail): None = the engine's plan-time rule (by
        # nms_topN_pre; bf16: M3D_BF16_SPARSE_HEADS=0 / 1 overrides it); the bundled form and a plan without a tail stay dense
        # whatever is asked
        if sparse_heads is None:
            sparse_heads = self.eng.sparse_heads_default(self.plan, conf.nms_topN_pre)
        self.sparse_heads = bool(sparse_heads) and bool(planar) and getattr(self.plan, "tail", None) is not None
        self.defer_3d = False                           # (PipelinedDetector: the 3-D size, depth and angle heads behind the NMS)
        self._rois = net.rois.to(dev)
        # refine mode: calibration / scale / image size of the batch whose detections the next replay refines
        self._meta = RefineMeta(self.batch, dev) if self.refine else None

    def _forward(self, start, end, buf=0, tail=False):
        """plan.ops[start:end]; tail: with the detection-only tail behind anchor_select (end = n_fwd), for a decode of
        conf.nms_topN_pre rows as it stands now."""
        if tail:
            bits = self.plan.named["score_bits"]
            self.plan.named["sparse_k"][0] = min(int(self.conf.nms_topN_pre), bits.shape[1])
        if self.u8_frame is None:
            self.plan.named["input_ptr"][0] = self.input.data_ptr()
            self.eng.run_plan(self.plan, start, end, tail)
            return
        # the stem launch reads (pointer, h, w) of the uint8 frames when it is ISSUED: capture bakes buffer `buf` into the graph
        self.plan.named["input_u8"][:] = [self.inputs_u8[buf].data_ptr(), self.u8_frame[0], self.u8_frame[1]]
        try:
            self.eng.run_plan(self.plan, start, end, tail)
        finally:
            self.plan.named["input_u8"][0] = 0

    def _select(self, rows, fill=None):
        """(aboxes, keep, num) of a detect_from_* -> (block, counts, refined rows or None).  fill(block, counts): what completes
        the selected rows of the block in place, in front of the refinement."""
        block, counts = select_block(*rows, self.conf)
        if fill is not None:
            fill(block, counts)
        if not self.refine:
            return block, counts, None
        # the block's rows are the kept rows + the count row (past counts[b]: refined to zeros); the scale factors were applied
        # inside the decode, before the NMS (lib/rpn_util.py:1504-1506), not here
        m = self._meta
        return block, counts, refine_rows(block, counts, m.p2, m.p2_inv, None, m.clip, *self._rargs)

    def _result(self, block, counts, refined, as_block):
        res = (block if as_block else block[:, :-1], counts)
        return res + (refined[:, :-1],) if self.refine else res


class PipelinedDetector(_Detector):
    def __init__(self, net, conf, batch, height, width, refine=False, score_thresh=0.75, step_r_init=0.3 * math.pi, r_lim=0.01,
                 u8_frame=None, planar=None, sparse_heads=None, defer_3d=None):
        planar = (os.environ.get("M3D_PIPE_PLANAR", "1") != "0") if planar is None else bool(planar)
        super().__init__(net, conf, batch, height, width, refine, score_thresh, step_r_init, r_lim, u8_frame, 2, sparse_heads, planar)
        self.planar = planar
        # the heads and the attention behind columns 8..12 of a row only at the pixels of the rows that survive the NMS, on the side
        # branch (plan.tail_pre / plan.post3d): None = whenever the sparse heads are on and the plan offers the split
        # (M3D_DEFER_3D=0: off), False = the one-part tail; a plan that does not offer it keeps that tail whatever is asked
        if defer_3d is None:
            defer_3d = os.environ.get("M3D_DEFER_3D", "1") != "0"
        self.defer_3d = bool(defer_3d) and self.sparse_heads and getattr(self.plan, "post3d", None) is not None
        if self.u8_frame is not None:
            # slot i: address of the pinned-host frames that the graph reading buffer i uploads into buffer i ^ 1 (0 = nothing)
            self._slots = torch.zeros(2, dtype=torch.int64).pin_memory()
            self._done = [torch.cuda.Event(), torch.cuda.Event()]      # the last replay of graph i finished (main stream)
            self._used = [False, False]
            self._queue = []                                           # fed, not yet submitted frame sets (kept alive here)
            self._cur = 0                                              # buffer the next submitted batch is read from
            self._primed = False                                       # buffer _cur holds the head of the queue
            self._inflight = [None, None]                              # frames a replay of graph i is uploading (kept alive)
            self._prime_ev = None                                      # behind feed()'s own copy of a batch nothing in flight uploads
        n = self.plan.named
        # planar form: the side branch must be done before the first launch that overwrites the planar staging
        # bundled form: detect(k-1) reads prob / bbox_* / score_bits; bundle_outputs (the last op) writes the first three, but with
        # SELECT_KEYS anchor_select of batch k already writes score_bits in the middle of the forward (that write ran
        # unordered against the side branch's top-k): join in front of the FIRST op that writes anything the side branch reads
        self.n_join = int(n["planar_first_op"]) if self.planar else min(self.n_fwd, int(n.get("score_bits_first_write_op", self.n_fwd)))
        self._check_no_write_beside_detect()
        # where the side branch forks off (experiment switch M3D_PIPE_FORK = op index; default: at the first launch).  In the bf16 graph
        # the persistent front end is stretched from 0.83 to 1.09 ms by detect(k-1) beside it (tools/graph_timeline.py), but forking
        # behind it moves the cost, it does not remove it: 10.48 / 10.58 / 10.61 / 10.52 ms for forks at op 0 / 1 / 2 / 3 on one lease
        # (fp32: 6.00 / 6.01 / 5.99 / 6.04, later forks worse) -- detect's 0.3 ms of mask arithmetic is work, not latency.
        fork = os.environ.get("M3D_PIPE_FORK")
        self.n_fork = min(int(fork) if fork is not None else int(n.get("pipe_fork_op", 0)), self.n_join)
        self._outs = (n["prob"], n["bbox_2d"], n["bbox_3d"])
        self._pending = False
        self._meta_next = None                          # (refine mode, host) the meta of the batch submitted last
        self._build()

    def _check_no_write_beside_detect(self):
        """No op of forward(k) in [0, n_join) may write a buffer that detect(k-1) reads: the ops that do are known by name
        (the heads and anchor_select write the planar staging / the sort keys, bundle_outputs the bundled tensors)."""
        n = self.plan.named
        first_writer = {"planar": int(n["planar_first_op"]), "keys": int(n.get("score_bits_first_write_op", self.n_fwd)),
                        "bundled": self.n_fwd}
        reads = ("planar", "keys") if self.planar else ("keys", "bundled")
        limit = min(first_writer[r] for r in reads)
        if self.n_join > limit:
            raise AssertionError("PipelinedDetector: join at op %d, but op %d of the next forward writes what detect reads (%s)"
                                 % (self.n_join, limit, first_writer))
        if self.defer_3d:
            # the side branch also runs plan.post3d of batch k-1: every map those launches read (the engine recorded them with
            # their first writers) must not be written by forward(k) in front of the join either
            for t, w in self.plan.post3d_reads:
                if w < self.n_join:
                    raise AssertionError("PipelinedDetector: join at op %d, but op %d of the next forward writes a map the deferred "
                                         "3-D launches read" % (self.n_join, w))

    def _detect(self):
        prob, b2, b3 = self._outs
        scale = self._meta.scale if self.refine else None
        if self.defer_3d:
            # 2-D top-k + NMS + selection, then the 3-D part of the forward at the survivors' pixels and their columns 8..12
            aboxes, keep, num, rows_out = detect_from_planar_2d(self.eng, self.plan, self._rois, self.conf, scale)

            def fill(block, counts):
                post_rows(self.plan, rows_out, keep, num, self.conf)
                self.eng.run_post3d(self.plan)
                fill_post_3d(self.eng, self.plan, self._rois, rows_out, keep, counts, block, self.conf)
            return self._select((aboxes, keep, num), fill)
        if self.planar:
            rows = detect_from_planar(self.eng, self.plan, self._rois, self.conf, scale)
        else:
            rows = detect_from_outputs(self.eng, self.plan, prob, b2, b3, self._rois, self.conf, scale)
        return self._select(rows)

    def _finish(self, buf=0):
        """The launches behind the join: the rest of the forward, then the key-only pass (planar) or the output bundling."""
        if self.planar:
            if self.n_join < self.n_fwd:
                self._forward(self.n_join, self.n_fwd, buf, "pre" if self.defer_3d else self.sparse_heads)
            if not self.plan.named.get("keys_by_select"):    # else anchor_select wrote them on the way (engine: SELECT_KEYS)
                score_keys_planar(self.eng, self.plan)
        else:
            self._forward(self.n_join, None, buf)

    def _capture_step(self, cap, side, buf):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            if self.n_fork:                          # launches of batch k in front of the fork (they do not share the chip well)
                self._forward(0, self.n_fork, buf)
            side.wait_stream(cap)                    # fork
            with torch.cuda.stream(side):
                outs = self._detect()                # batch k-1
                if self.u8_frame is not None:        # frames of batch k+1: pinned host -> the OTHER input buffer, as a kernel
                    _hip.check(_hip.lib().m3d_upload_indirect(
                        ctypes.c_void_p(self._slots.data_ptr() + 8 * buf), ctypes.c_void_p(self._u8_flat[buf ^ 1].data_ptr()),
                        self._u8_bytes, ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
            self._forward(self.n_fork, self.n_join, buf)   # batch k, everything in front of the first write of what the side branch reads
            cap.wait_stream(side)                    # join: outputs may now be overwritten
            self._finish(buf)
        return g, outs

    def _build(self):
        cap, side = torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)
        cap.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(cap), torch.no_grad():
            self._forward(0, self.n_join)                # warm-up outside capture: plan buffers, allocator pools,
            self._finish()                               # kernel attributes, zero page
            self._detect()
            torch.cuda.synchronize(self.dev)
            self.graph, (self._block, self._counts, self._refined) = self._capture_step(cap, side, 0)
            if self.u8_frame is not None:                # second input buffer: its own graph, its own result tensors
                self._graphs = [self.graph, None]
                self._results = [(self._block, self._counts, self._refined), None]
                self._graphs[1], self._results[1] = self._capture_step(cap, side, 1)
            # tail graph for flush(): detect only
            self.tail = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.tail, stream=cap):
                self._tblock, self._tcounts, self._trefined = self._detect()
        torch.cuda.current_stream(self.dev).wait_stream(cap)

    def _upload_meta(self):
        """Calibration of the batch submitted LAST -> the device buffers the refinement of the next replay reads."""
        if self._meta_next is not None:
            self._meta.upload(self._meta_next)

    # ---- fed-input form ---------------------------------------------------------------------------------------------------------
    def feed(self, frames):
        """Queue one batch of uint8 BGR frames [B, h, w, 3] in PINNED host memory (a device tensor works too).  Nothing is copied
        here: the graph of the batch submitted BEFORE this one uploads it (the first batch is uploaded right away) -- an
        asynchronous read of this tensor.  The tensor must stay unchanged until the step_fed() that SUBMITS it has returned:
        that call waits (on the host, behind its own replay launch, so the device never idles) for the replay / copy that
        uploaded the batch.  A ring of two pinned buffers written in the order feed, step_fed, feed, step_fed, ... is therefore
        safe.  At most two batches can be queued."""
        if self.u8_frame is None:
            raise RuntimeError("feed() needs PipelinedDetector(..., u8_frame=(h, w))")
        if len(self._queue) >= 2:
            raise RuntimeError("feed(): two batches are queued already; call step_fed()")
        if frames.dtype != torch.uint8 or tuple(frames.shape) != tuple(self.inputs_u8[0].shape) or not frames.is_contiguous():
            raise RuntimeError("feed(): contiguous uint8 frames of shape %s expected, got %s %s"
                               % (tuple(self.inputs_u8[0].shape), frames.dtype, tuple(frames.shape)))
        if not (frames.is_cuda or frames.is_pinned()):
            raise RuntimeError("feed(): the frames must be in pinned host memory (tensor.pin_memory()) or on the device")
        self._queue.append(frames)
        if not self._primed:                                     # nothing in flight names this batch: upload it now
            self.inputs_u8[self._cur].copy_(frames, non_blocking=True)
            self._prime_ev = torch.cuda.Event()                  # the copy reads the pinned tensor asynchronously
            self._prime_ev.record(torch.cuda.current_stream(self.dev))
            self._primed = True

    def step_fed(self, as_block=False):
        """Submit the oldest queued batch; its graph also uploads the next queued batch (if any) into the other buffer.  Returns
        (dets, counts) of the batch submitted before it (None for the first call).  The returned tensors belong to the graph of
        that input buffer and are overwritten two steps later."""
        if not self._queue:
            raise RuntimeError("step_fed(): no batch was fed")
        i = self._cur
        self._queue.pop(0)
        nxt = self._queue[0] if self._queue else None
        if self._used[i]:
            self._done[i].synchronize()          # (host) the previous replay of this graph has read its slot
        self._slots[i] = nxt.data_ptr() if nxt is not None else 0
        self._inflight[i] = nxt
        main = torch.cuda.current_stream(self.dev)
        had = self._pending
        self._graphs[i].replay()
        self._done[i].record(main)
        # The batch submitted here was uploaded by the PREVIOUS replay (graph i ^ 1, side branch) or by feed()'s own copy: wait
        # for that read of the caller's pinned tensor -- behind this replay's launch, so one replay is always queued on the
        # device -- and the documented lifetime ("unchanged until the step_fed() that submits it has returned") holds for a
        # two-deep ring as well (_done[i] above is two replays back and did not cover it).
        if self._used[i ^ 1]:
            self._done[i ^ 1].synchronize()
        if self._prime_ev is not None:
            self._prime_ev.synchronize()
            self._prime_ev = None
        self._used[i] = True
        self._pending = True
        self._cur ^= 1
        self._primed = nxt is not None           # the replay uploads it into the buffer the next step reads
        if not had:
            return None
        block, counts, _ = self._results[i]
        return (block if as_block else block[:, :-1], counts)

    def step(self, x=None, as_block=False, meta=None):
        """Submit batch k (copied into ``self.input`` unless x is None = already written there); returns
        (dets, counts) of batch k-1, or None for the first call.  Returned tensors are overwritten by the next step.
        as_block: return the [B, nms_topN_post + 1, 14] gather block (m3dssd_amd.dist.gather_block) instead of dets.
        refine mode: meta = {"p2": [B, 4, 4] (or [4, 4]), "scale": [B] or None, "clip_wh": [B, 2] or None} of batch k; the
        return value gains a third element, the refined rows [B, nms_topN_post, 16] (float64) of batch k-1."""
        if self.u8_frame is not None:
            if self.refine:
                raise NotImplementedError("refine=True with fed uint8 frames: use step() with float frames")
            if x is not None:
                self.feed(x)
            return self.step_fed(as_block)
        if x is not None:
            self.input.copy_(x)
        had = self._pending
        if self.refine:
            if meta is None:
                raise RuntimeError("PipelinedDetector(refine=True).step needs the batch's meta (p2, scale, clip_wh)")
            self._upload_meta()                      # of batch k-1: what this replay's refinement reads
            self._meta_next = meta
        self.graph.replay()
        self._pending = True
        if not had:
            return None
        return self._result(self._block, self._counts, self._refined, as_block)

    def flush(self, as_block=False):
        """Detections of the last submitted batch."""
        if not self._pending:
            return None
        if self.refine:
            self._upload_meta()
            self._meta_next = None
        self.tail.replay()
        self._pending = False
        return self._result(self._tblock, self._tcounts, self._trefined, as_block)


# FrameDetector(topk_wgs=None): the multi-workgroup top-k up to this batch size, the single-workgroup kernel (one workgroup per
# image) above it.  The rule for moving it is a measurement: the kernel leg of tools/latency_frame.py (profiles/latency_frame.jsonl)
# has to show the multi-workgroup kernel's p50 below the single-workgroup one by more than the spread of the latter against itself.
# NOT MEASURED yet ("Single frame"), so the default stays the single-workgroup kernel at every batch size.
FRAME_MW_MAX_BATCH = 0


class FrameDetector(_Detector):
    """Single-frame mode: ``detect(x)`` returns the detections of THIS x.

    One captured hipGraph per instance holds the whole planar-form forward of the plan, the key pass (where the plan does not write
    the sort keys itself), top-k + decode from the planar staging, NMS, row selection and -- ``refine=True`` -- the 3-D refinement
    of ``test_kitti_3d`` (``m3d_refine_3d_ex``).  Nothing is deferred and there is no side stream: the only branches are the ones
    ``run_plan`` emits under capture.  Results are those of ``detect_batch(net, x, conf, scale=...)`` (+ ``refine_detections``),
    bit for bit (tests/test_gpu_frame_detector.py); a caller with a stream of batches who can take the result one batch late gets
    more frames per second from ``PipelinedDetector``.

    ``u8_frame=(h, w)``: x is uint8 BGR [B, h, w, 3] (device tensor or pinned host memory), copied on the current stream into the
    device buffer the stem reads (padding, normalisation and BGR->RGB happen in its loads).
    ``topk_wgs``: None = the library's choice (FRAME_MW_MAX_BATCH), 1 = the single-workgroup ``m3d_topk_decode_planar``, any other
    positive value = workgroups per image of ``m3d_topk_decode_planar_mw``."""

    def __init__(self, net, conf, height, width, batch=1, refine=False, score_thresh=0.75, step_r_init=0.3 * math.pi, r_lim=0.01,
                 u8_frame=None, topk_wgs=None, sparse_heads=None):
        if topk_wgs is not None and int(topk_wgs) < 1:
            raise ValueError("topk_wgs must be None or a positive number of workgroups per image, got %r" % (topk_wgs,))
        super().__init__(net, conf, batch, height, width, refine, score_thresh, step_r_init, r_lim, u8_frame, 1, sparse_heads)
        if topk_wgs is None:
            self.topk_wgs = 0 if self.batch <= FRAME_MW_MAX_BATCH else 1       # 0: m3d_topk_decode_planar_mw picks the count
        else:
            self.topk_wgs = int(topk_wgs)
        self._build()

    def _run(self):
        """Forward, keys, detection (and refinement) of what ``self.input`` holds, on the current stream."""
        self._forward(0, self.n_fwd, 0, self.sparse_heads)
        if not self.plan.named.get("keys_by_select"):       # else anchor_select wrote them on the way (engine: SELECT_KEYS)
            score_keys_planar(self.eng, self.plan)
        scale = self._meta.scale if self.refine else None
        if self.topk_wgs == 1:
            rows = detect_from_planar(self.eng, self.plan, self._rois, self.conf, scale)
        else:
            rows = detect_from_planar_mw(self.eng, self.plan, self._rois, self.conf, scale, self.topk_wgs or None)
        return self._select(rows)

    def _build(self):
        cap = torch.cuda.Stream(self.dev)
        cap.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(cap), torch.no_grad():
            self._run()                                     # warm-up outside capture: plan buffers, allocator pools, kernel attributes
            torch.cuda.synchronize(self.dev)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=cap):
                self._block, self._counts, self._refined = self._run()
        torch.cuda.current_stream(self.dev).wait_stream(cap)

    def detect(self, x, meta=None, as_block=False):
        """Detections of x: (dets [B, nms_topN_post, 14], counts [B] int32), with refine=True also the refined rows
        [B, nms_topN_post, 16] (float64).  Device tensors, queued on the current stream; the host is not synchronised.  The tensors
        belong to the graph and are overwritten by the next detect(): clone what has to outlive it.
        x: float32 [B, 3, height, width], or with u8_frame uint8 BGR [B, h, w, 3] on the device or in pinned host memory.
        refine=True: meta = {"p2": [B, 4, 4] (or [4, 4]), "scale": [B] or None, "clip_wh": [B, 2] or None} of THIS x.
        as_block: return the [B, nms_topN_post + 1, 14] gather block (m3dssd_amd.dist.gather_block) instead of dets."""
        want = torch.uint8 if self.u8_frame is not None else torch.float32
        if not torch.is_tensor(x) or x.dtype != want or tuple(x.shape) != tuple(self.input.shape):
            raise RuntimeError("FrameDetector.detect: %s frames of shape %s expected, got %s %s"
                               % (str(want).replace("torch.", ""), tuple(self.input.shape), getattr(x, "dtype", type(x).__name__),
                                  tuple(getattr(x, "shape", ()))))
        if self.u8_frame is not None and not (x.is_cuda or x.is_pinned()):
            raise RuntimeError("FrameDetector.detect: the uint8 frames must be in pinned host memory (tensor.pin_memory()) or on the device")
        if self.refine:
            if meta is None:
                raise RuntimeError("FrameDetector(refine=True).detect needs the frame's meta (p2, scale, clip_wh)")
            self._meta.upload(meta)
        self.input.copy_(x, non_blocking=True)
        self.graph.replay()
        return self._result(self._block, self._counts, self._refined, as_block)
