"""The argument path of the patch ops, pinned message by message: every refusal below fires on CPU tensors before any launch,
and the strings are literals taken from the code as it stood before the wrappers were put on one shared stanza, so a change of
a message, of the op name it carries or of the order in which two refusals fire shows up here.  No GPU.

The table: for the three ops with a per-reference-patch tensor (ref_weight, ref_radius) a wrong dtype, a wrong shape and a bad
value; for each of the ten wrappers with a patch argument a patch of 2 entries, a stride of 0 and a volume of the wrong dtype,
where the wrapper has such an argument (patch_match has no stride; patch_nn_counts takes shapes, not volumes).  A wrapper that
sees a CPU tensor before it looks at the stride (patch_proj_hist) says that instead, which is pinned too.  volume_resize_u8
takes its volume through the same check and is listed with it."""
import pytest
import torch

from hp_vae_gan_amd import ops

P3, P2, ONE, Z = (1, 3, 3), (3, 3), (1, 1, 1), (1, 0, 1)
Q = torch.zeros(2, 9, 10, 3, dtype=torch.uint8)
R = torch.zeros(2, 8, 9, 3, dtype=torch.uint8)           # patch grid 2 x 6 x 7 = 84
QI, RI = Q[0], R[0]                                      # images: ref patch grid 6 x 7 = 42
M = torch.zeros(2, 9, 10, dtype=torch.uint8)
W = torch.ones(84)
RAD = torch.ones(84, dtype=torch.int32)
NN = torch.zeros(2 * 7 * 8, dtype=torch.int32)
DIRS = torch.ones(2, 27, dtype=torch.int8)
F = Q.float()


def _w(v):
    w = W.clone()
    w[5] = v
    return w


COUNTS = "hpvg_patchnn_counts failed: HPVG_ERR_ARG"
CASES = [
    # ---- the per-reference-patch tensors
    ("weighted-dtype", lambda: ops.patch_nn_weighted(Q, R, W.double(), P3),
     "patch_nn_weighted: ref_weight must be float32 [84] or (2, 6, 7) on cpu, got torch.float64 (84,) on cpu"),
    ("weighted-shape", lambda: ops.patch_nn_weighted(Q, R, W[:83], P3),
     "patch_nn_weighted: ref_weight must be float32 [84] or (2, 6, 7) on cpu, got torch.float32 (83,) on cpu"),
    ("weighted-image-shape", lambda: ops.patch_nn_weighted(QI, RI, W, P3),
     "patch_nn_weighted: ref_weight must be float32 [42] or (6, 7) on cpu, got torch.float32 (84,) on cpu"),
    ("weighted-not-a-tensor", lambda: ops.patch_nn_weighted(Q, R, [1.0] * 84, P3),
     "patch_nn_weighted: ref_weight must be float32 [84] or (2, 6, 7) on cpu, got <class 'list'> () on None"),
    ("weighted-zero", lambda: ops.patch_nn_weighted(Q, R, _w(0.0), P3), "patch_nn_weighted: every ref_weight must be finite and > 0"),
    ("weighted-inf", lambda: ops.patch_nn_weighted(Q, R, _w(float("inf")), P3),
     "patch_nn_weighted: every ref_weight must be finite and > 0"),
    ("match-dtype", lambda: ops.patch_match(Q, R, P3, 2, ref_weight=W.double()),
     "patch_match: ref_weight must be float32 [84] or (2, 6, 7) on cpu, got torch.float64 (84,) on cpu"),
    ("match-shape", lambda: ops.patch_match(Q, R, P3, 2, ref_weight=W.reshape(2, 42)),
     "patch_match: ref_weight must be float32 [84] or (2, 6, 7) on cpu, got torch.float32 (2, 42) on cpu"),
    ("match-zero", lambda: ops.patch_match(Q, R, P3, 2, ref_weight=_w(0.0)), "patch_match: every ref_weight must be finite and > 0"),
    ("match-inf", lambda: ops.patch_match(Q, R, P3, 2, ref_weight=_w(float("inf"))),
     "patch_match: every ref_weight must be finite and > 0"),
    ("ball-dtype", lambda: ops.patch_ball_count(Q, R, RAD.long(), P3),
     "patch_ball_count: ref_radius must be int32 [84] or (2, 6, 7) on cpu, got torch.int64 (84,) on cpu"),
    ("ball-shape", lambda: ops.patch_ball_count(Q, R, RAD.reshape(6, 14), P3),
     "patch_ball_count: ref_radius must be int32 [84] or (2, 6, 7) on cpu, got torch.int32 (6, 14) on cpu"),
    ("ball-negative", lambda: ops.patch_ball_count(Q, R, RAD - 2, P3), "patch_ball_count: every ref_radius must be >= 0"),
    # ---- a patch of 2 entries
    ("counts-patch2", lambda: ops.patch_nn_counts((2, 9, 10), (2, 8, 9), P2), "patch_nn: patch must have 3 entries (t, h, w), got 2"),
    ("nn-patch2", lambda: ops.patch_nn(Q, R, P2), "patch_nn: patch must have 3 entries (t, h, w), got 2"),
    ("weighted-patch2", lambda: ops.patch_nn_weighted(Q, R, W, P2), "patch_nn_weighted: patch must have 3 entries (t, h, w), got 2"),
    ("match-patch2", lambda: ops.patch_match(Q, R, P2, 2), "patch_match: patch must have 3 entries (t, h, w), got 2"),
    ("subset-patch2", lambda: ops.patch_nn_subset(Q, R, P2), "patch_nn_subset: patch must have 3 entries (t, h, w), got 2"),
    ("mask-patch2", lambda: ops.patch_mask_count(M, P2), "patch_mask_count: patch must have 3 entries (t, h, w), got 2"),
    ("knn-patch2", lambda: ops.patch_knn_self(Q, P2, 3), "patch_knn_self: patch must have 3 entries (t, h, w), got 2"),
    ("ball-patch2", lambda: ops.patch_ball_count(Q, R, RAD, P2), "patch_ball_count: patch must have 3 entries (t, h, w), got 2"),
    ("vote-patch2", lambda: ops.patch_vote(R, NN, P2, (2, 9, 10), Q), "patch_vote: patch must have 3 entries (t, h, w), got 2"),
    ("hist-patch2", lambda: ops.patch_proj_hist(Q, P2, DIRS), "patch_proj_hist: patch must have 3 entries (t, h, w), got 2"),
    # ---- a stride of 0
    ("counts-stride0", lambda: ops.patch_nn_counts((2, 9, 10), (2, 8, 9), P3, Z), COUNTS),
    ("nn-stride0", lambda: ops.patch_nn(Q, R, P3, qstride=Z), COUNTS),
    ("weighted-stride0", lambda: ops.patch_nn_weighted(Q, R, W, P3, rstride=Z), COUNTS),
    ("subset-stride0", lambda: ops.patch_nn_subset(Q, R, P3, qstride=Z), COUNTS),
    ("mask-stride0", lambda: ops.patch_mask_count(M, P3, Z), COUNTS),
    ("knn-stride0", lambda: ops.patch_knn_self(Q, P3, 3, Z), COUNTS),
    ("ball-stride0", lambda: ops.patch_ball_count(Q, R, RAD, P3, rstride=Z), COUNTS),
    ("vote-stride0", lambda: ops.patch_vote(R, NN, P3, (2, 9, 10), Q, qstride=Z), "hpvg_patch_vote_counts failed: HPVG_ERR_ARG"),
    ("hist-stride0", lambda: ops.patch_proj_hist(Q, P3, DIRS, Z),
     "patch_proj_hist: vol on cpu, dirs on cpu; both must be on one MI355X device"),
    # ---- a volume of the wrong dtype
    ("nn-dtype", lambda: ops.patch_nn(F, R, P3), "patch_nn: query must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("weighted-dtype-vol", lambda: ops.patch_nn_weighted(Q, R.float(), W, P3),
     "patch_nn_weighted: ref must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 8, 9, 3)"),
    ("match-dtype-vol", lambda: ops.patch_match(F, R, P3, 2),
     "patch_match: query must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("subset-dtype", lambda: ops.patch_nn_subset(F, R, P3),
     "patch_nn_subset: query must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("mask-dtype", lambda: ops.patch_mask_count(M.float(), P3),
     "patch_mask_count: mask must be uint8 [T,H,W] or [H,W], got torch.float32 (2, 9, 10)"),
    ("knn-dtype", lambda: ops.patch_knn_self(F, P3, 3),
     "patch_knn_self: vol must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("ball-dtype-vol", lambda: ops.patch_ball_count(F, R, RAD, P3),
     "patch_ball_count: query must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("vote-dtype", lambda: ops.patch_vote(R, NN, P3, (2, 9, 10), F),
     "patch_vote: fallback must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("hist-dtype", lambda: ops.patch_proj_hist(F, P3, DIRS),
     "patch_proj_hist: vol must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("resize-dtype", lambda: ops.volume_resize_u8(F, (1, 2, 2)),
     "volume_resize_u8: the volume must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("resize-not-a-tensor", lambda: ops.volume_resize_u8([1, 2], (1, 2, 2)),
     "volume_resize_u8: the volume must be uint8 [T,H,W,3] or [H,W,3], got <class 'list'> ()"),
    # ---- the order of two refusals: the volumes come before the patch, the patch before the per-reference tensor,
    # ---- patch_match's ring flags between the volumes and the patch, the k of patch_knn_self after the geometry
    ("order-vol-patch", lambda: ops.patch_ball_count(F, R, RAD.long(), P2),
     "patch_ball_count: query must be uint8 [T,H,W,3] or [H,W,3], got torch.float32 (2, 9, 10, 3)"),
    ("order-patch-weight", lambda: ops.patch_nn_weighted(Q, R, W.double(), P2),
     "patch_nn_weighted: patch must have 3 entries (t, h, w), got 2"),
    ("order-match-wrap-patch", lambda: ops.patch_match(Q, R, P2, 2, qwrap=(2, 0, 0)),
     "patch_match: qwrap must be three flags (t, h, w), each 0 or 1, got (2, 0, 0)"),
    ("order-vote-shape-patch", lambda: ops.patch_vote(R, NN, P2, (2, 9, 9), Q),
     "patch_vote: out_shape (2, 9, 9) is not the fallback's (2, 9, 10)"),
    ("order-knn-stride-k", lambda: ops.patch_knn_self(Q, P3, 9, Z), COUNTS),
    ("knn-k", lambda: ops.patch_knn_self(Q, P3, 9), "patch_knn_self: k must be an int in [1, 8], got 9"),
    ("subset-sel", lambda: ops.patch_nn_subset(Q, R, P3, qsel=torch.zeros(3)),
     "patch_nn_subset: qsel must be a non-empty 1-D int32 tensor on cpu, got torch.float32 (3,) on cpu"),
    ("mixed-rank", lambda: ops.patch_nn(Q, RI, P3), "patch_nn: query and ref must both be volumes or both be images"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_refusal_and_its_message(case):
    _, fn, want = case
    with pytest.raises(RuntimeError) as e:
        fn()
    assert str(e.value) == want
