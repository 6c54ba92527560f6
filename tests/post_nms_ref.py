"""Host-side restatements (numpy) for the tests of the heads that run behind the NMS: the survivor pixel list of ``m3d_post_rows``
and the cases its tests share.  Imported by tests/test_post_nms_heads_host.py and tests/test_gpu_post_nms_heads.py; no GPU here."""
import numpy as np


def post_rows_ref(rows_out, keep, num_keep, post, HW):
    """rows_out [B][n] staging rows of the decoded rows, keep [B][n] kept positions (entries at or past num_keep[b] are never
    looked at), num_keep [B] -> the distinct pixels b * HW + rows_out[b][keep[b][j]] % HW of the first min(num_keep[b], post)
    kept rows of every image, ascending (int32)."""
    rows_out, keep, num_keep = np.asarray(rows_out), np.asarray(keep), np.asarray(num_keep)
    pix = []
    for b in range(rows_out.shape[0]):
        cnt = min(int(num_keep[b]), int(post))
        pix += [b * HW + int(rows_out[b, int(keep[b, j])]) % HW for j in range(cnt)]
    return np.unique(np.asarray(pix, dtype=np.int64)).astype(np.int32)


def post_rows_case(B=3, HW=128, A=4, n=100, seed=0):
    """(rows_out [B][n], keep [B][n], num_keep [B]) int32 with, for post in {1, 5, 40}:
      image 0: 7 kept rows; the first two are the same pixel under different anchors, and the pixels do not ascend with j
      image 1: no kept row
      image 2: 60 kept rows (more than every post), again with a pixel held twice among the first five
    keep entries at or past num_keep hold a position far outside [0, n): they must not be read."""
    assert B == 3 and n >= 60 and A >= 4
    g = np.random.RandomState(seed)
    rows_out = np.stack([g.permutation(A * HW)[:n] for _ in range(B)]).astype(np.int32)
    keep = np.full((B, n), 1 << 28, dtype=np.int32)
    num = np.array([7, 0, 60], dtype=np.int32)
    keep[0, :7] = np.sort(g.permutation(n)[:7])
    keep[2, :60] = np.sort(g.permutation(n)[:60])
    # one pixel twice, under anchors 1 and 3, in the first two kept rows; a high pixel in front of low ones
    rows_out[0, keep[0, 0]] = 1 * HW + 117
    rows_out[0, keep[0, 1]] = 3 * HW + 117
    rows_out[0, keep[0, 2]] = 0 * HW + 5
    rows_out[0, keep[0, 3]] = 2 * HW + 60
    rows_out[2, keep[2, 0]] = 2 * HW + 90
    rows_out[2, keep[2, 3]] = 0 * HW + 90
    rows_out[2, keep[2, 4]] = 1 * HW + 2
    return rows_out, keep, num
