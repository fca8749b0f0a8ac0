"""Layout terms of the reward, host side (no GPU): the numpy restatement (tests/layout_ref.py) against the recorded results of the
reference's compute_maximum_iou / compute_docsim (tests/golden/layout_ref.npz, tools/make_layout_goldens.py), the packing of
layouts for gl_layout_reward, the nearest-label step of RewardModel on a stub text tower, and the new entries of the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import layout_ref as lr
from layoutllm_t2i_amd import _lib, reward
from layoutllm_t2i_amd.reward import COCO_LABELS, MAX_BOXES, RewardModel, layout_terms, pack_layouts

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layout_ref.npz")
Z = np.load(GOLD)
NAMES, GT, PRED, MIOU, DOCSIM = lr.unpack(Z)


def close(got, want, tol=1e-13):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= tol * max(1.0, abs(want))


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("ci", range(len(NAMES)), ids=NAMES)
def test_restatement_reproduces_the_recorded_reference_results(ci):
    """float64 numpy on both sides, the same operations per entry: 1e-13 leaves room for the order of the assignment's sum only"""
    assert close(lr.maximum_iou(GT[ci], PRED[ci]), MIOU[ci]), (NAMES[ci], lr.maximum_iou(GT[ci], PRED[ci]), MIOU[ci])
    assert close(lr.docsim(GT[ci], PRED[ci]), DOCSIM[ci]), (NAMES[ci], lr.docsim(GT[ci], PRED[ci]), DOCSIM[ci])


def test_golden_file_holds_the_cases_the_kernel_is_tested_on():
    sizes = {n: (int(a), int(b)) for n, a, b in zip(NAMES, Z["n_gt"], Z["n_pred"])}
    for name, want in (("1x1", (1, 1)), ("1x4", (1, 4)), ("4x1", (4, 1)), ("3x3", (3, 3)), ("5x3", (5, 3)), ("3x5", (3, 5)), ("30x30_one_label", (30, 30)),
                       ("30x28_five_labels", (30, 28)), ("64x64", (64, 64)), ("64x62", (64, 62)), ("count_plus3", (6, 3)), ("count_minus3", (3, 6)),
                       ("count_plus2", (6, 4)), ("count_minus2", (4, 6)), ("empty_prediction_3", (3, 0)), ("empty_prediction_2", (2, 0))):
        assert sizes[name] == want, name
    v = dict(zip(NAMES, zip(MIOU, DOCSIM)))
    assert v["disjoint_labels"] == (0.0, 0.0) and v["count_plus3"][1] == 0.0 and v["count_minus3"][1] == 0.0
    assert v["count_plus2"][1] > 0.1 and v["count_minus2"][1] > 0.1 and v["empty_prediction_2"] == (0.0, 0.0)
    assert np.isnan(v["zero_area_pair"][0]) and v["zero_area_pair"][1] > 0.1 and int(np.isnan(MIOU).sum()) == 1
    assert len(set(Z["labels_gt"][NAMES.index("30x28_five_labels")][:30].tolist())) == 5
    # the scramble decides: the recorded value is not the true matching's wherever the matrix is rectangular with both sides >= 2
    for name in ("5x3", "3x5", "64x62", "30x28_five_labels", "count_plus2"):
        i = NAMES.index(name)
        assert abs(Z["miou_true_matching"][i] - MIOU[i]) > 1e-6 and abs(Z["docsim_true_matching"][i] - DOCSIM[i]) > 1e-6, name
        assert close(lr.maximum_iou(GT[i], PRED[i], lr.true_matrix), Z["miou_true_matching"][i])
    i = NAMES.index("negative_wh")
    assert (PRED[i][0][:, 2] * PRED[i][0][:, 3] < 0).sum() == 1


def test_brute_force_and_hungarian_agree():
    rng = np.random.default_rng(0)
    for t in range(60):
        n, m = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        mat = rng.uniform(0.0, 1.0, (n, m))
        if t % 4 == 0:
            mat = np.round(mat * 2) / 2                       # exact ties
        if t % 5 == 0:
            mat[rng.uniform(size=mat.shape) < 0.4] = 0.0      # other-label zeros
        best, second = lr.brute_force_max(mat)
        assert second <= best and abs(lr.hungarian_max(mat) - best) <= 1e-14 * max(1.0, abs(best)), (n, m, t)
    # and on the matrices of the golden cases where both apply
    for ci, name in enumerate(NAMES):
        (b1, c1), (b2, c2) = GT[ci], PRED[ci]
        N, M = len(b1), len(b2)
        if 0 < min(N, M) <= lr.BRUTE_MAX and max(N, M) <= 8 and name != "zero_area_pair":
            mat = lr.flat_matrix(lambda a, b: lr.bbox_sim(b1[a], c1[a], b2[b], c2[b]), N, M)
            assert abs(lr.hungarian_max(mat) - lr.brute_force_max(mat)[0]) <= 1e-14, name


def test_flat_fill_is_the_transpose_when_square_and_a_scramble_otherwise():
    f = lambda a, b: 10.0 * a + b
    assert np.array_equal(lr.flat_matrix(f, 3, 3), lr.true_matrix(f, 3, 3).T)
    assert np.array_equal(lr.flat_matrix(f, 1, 4), lr.true_matrix(f, 1, 4)) and np.array_equal(lr.flat_matrix(f, 4, 1), lr.true_matrix(f, 4, 1))
    got = lr.flat_matrix(f, 3, 2)                              # k -> f(k % 3, k // 3), rows of 2
    assert got.tolist() == [[0.0, 10.0], [20.0, 1.0], [11.0, 21.0]]


# ------------------------------------------------------------------------------------------- packing
def test_pack_layouts_pads_counts_and_casts():
    boxes, labels, counts = pack_layouts([([[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8]], [3, 79]), (np.zeros((0, 4)), np.zeros(0, np.int64)),
                                          (np.arange(256, dtype=np.float32).reshape(64, 4), np.arange(64)), ([], [])])
    assert boxes.shape == (4, MAX_BOXES, 4) and boxes.dtype == np.float64 and boxes.flags["C_CONTIGUOUS"]
    assert labels.shape == (4, MAX_BOXES) and labels.dtype == np.int32 and counts.dtype == np.int32 and counts.tolist() == [2, 0, 64, 0]
    assert boxes[0, :2].tolist() == [[0.1, 0.2, 0.3, 0.4], [0.5, 0.6, 0.7, 0.8]] and not boxes[0, 2:].any() and labels[0, :3].tolist() == [3, 79, 0]
    assert not boxes[1].any() and not labels[1].any() and labels[2].tolist() == list(range(64)) and boxes[2, 63].tolist() == [252.0, 253.0, 254.0, 255.0]


def test_pack_layouts_and_layout_terms_refuse_what_the_kernel_cannot_take():
    ok = (np.zeros((2, 4)), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="at most 64"):
        pack_layouts([ok, (np.zeros((65, 4)), np.zeros(65, np.int64))])
    with pytest.raises(ValueError, match=r"expected \[n, 4\]"):
        pack_layouts([(np.zeros((2, 3)), np.zeros(2, np.int64))])
    with pytest.raises(ValueError, match=r"expected \[n, 4\]"):
        pack_layouts([(np.zeros(8), np.zeros(2, np.int64))])
    with pytest.raises(ValueError, match="2 boxes but labels"):
        pack_layouts([(np.zeros((2, 4)), np.zeros(3, np.int64))])
    # layout_terms refuses before it touches a device
    with pytest.raises(ValueError, match="2 ground-truth layouts but 1"):
        layout_terms([ok, ok], [ok], "cpu")
    with pytest.raises(ValueError, match="layout 1: empty ground-truth layout"):
        layout_terms([ok, (np.zeros((0, 4)), np.zeros(0, np.int64))], [ok, ok], "cpu")
    with pytest.raises(ValueError, match="at most 64"):
        layout_terms([ok], [(np.zeros((65, 4)), np.zeros(65, np.int64))], "cpu")
    with pytest.raises(ValueError, match=r"expected \[n, 4\]"):
        layout_terms([(np.zeros((2, 5)), np.zeros(2, np.int64))], [ok], "cpu")
    with pytest.raises(ValueError, match="no layouts"):
        layout_terms([], [], "cpu")


# ------------------------------------------------------------------------------------------- labels
class StubTower:
    """get_text_features of a text tower whose feature is a fixed direction per first token id"""

    def __init__(self, D=8):
        self.calls, self.rows = 0, []
        g = torch.Generator().manual_seed(0)
        self.table = torch.randn(200, D, generator=g)

    def get_text_features(self, input_ids, attention_mask=None):
        self.calls += 1
        ids = torch.as_tensor(input_ids)
        self.rows.append(int(ids.shape[0]))
        return self.table[ids[:, 0]] * (1.0 + ids[:, 0:1].float())        # unnormalised on purpose


LABELS = ["person", "car", "dog", "chair"]
WORD_ID = {"person": 0, "car": 1, "dog": 2, "chair": 3, "puppy": 102, "automobile": 101, "sofa": 103}


def stub_model():
    rm = RewardModel.__new__(RewardModel)               # the label methods need a text tower only
    rm.towers, rm.device = StubTower(), torch.device("cpu")
    rm.towers.table[102] = rm.towers.table[2] + 0.05 * rm.towers.table[1]      # puppy ~ dog
    rm.towers.table[101] = -3.0 * rm.towers.table[0] + 4.0 * rm.towers.table[1]  # automobile ~ car
    rm.towers.table[103] = rm.towers.table[3] * 0.2                              # sofa ~ chair
    return rm


def tokenize(words):
    tokenize.seen.append(list(words))
    return torch.tensor([[WORD_ID[w], 99] for w in words]), torch.ones(len(words), 2, dtype=torch.long)


def test_nn_close_set_and_label_to_id_on_a_stub_tower():
    rm = stub_model()
    with pytest.raises(RuntimeError, match="emb_labels"):
        rm.label_to_id([([[0, 0, 1, 1]], ["car"])])
    tokenize.seen = []
    emb = rm.emb_labels(LABELS, *tokenize(LABELS))
    assert emb.shape == (4, 8) and torch.allclose(emb.norm(dim=-1), torch.ones(4)) and rm.label2index == {l: i for i, l in enumerate(LABELS)}
    assert rm.towers.calls == 1
    b = lambda n: [[0.1 * i, 0.1, 0.5, 0.6] for i in range(n)]
    layouts = [(b(3), ["car", "puppy", "person"]), (b(2), ["puppy", "automobile"]), (b(0), []), (b(3), ["sofa", "puppy", "dog"])]
    tokenize.seen = []
    closed = rm.nn_close_set(layouts, tokenize)
    # one tower call for the batch, every distinct unknown label once, in order of first appearance
    assert rm.towers.calls == 2 and rm.towers.rows[-1] == 3 and tokenize.seen == [["puppy", "automobile", "sofa"]]
    assert [l for _, l in closed] == [["car", "dog", "person"], ["dog", "car"], [], ["chair", "dog", "dog"]]
    assert all(c[0] is l[0] for c, l in zip(closed, layouts))              # boxes pass through
    ids = rm.label_to_id(closed)
    assert [i.tolist() for _, i in ids] == [[1, 2, 0], [2, 1], [], [3, 2, 2]] and all(isinstance(bx, np.ndarray) for bx, _ in ids)
    assert ids[0][0].shape == (3, 4)
    # known labels only: no tower call, no tokenizer call
    tokenize.seen = []
    assert rm.nn_close_set([(b(2), ["dog", "chair"])], tokenize)[0][1] == ["dog", "chair"] and rm.towers.calls == 2 and tokenize.seen == []
    with pytest.raises(KeyError):
        rm.label_to_id([(b(1), ["puppy"])])
    with pytest.raises(ValueError, match="4 labels but 2 token rows"):
        rm.emb_labels(LABELS, *tokenize(LABELS[:2]))


def test_coco_label_table_is_the_reference_order():
    assert len(COCO_LABELS) == 80 == len(set(COCO_LABELS))
    assert COCO_LABELS[0] == "person" and COCO_LABELS[9] == "traffic light" and COCO_LABELS[39] == "bottle" and COCO_LABELS[79] == "toothbrush"
    assert COCO_LABELS.index("dining table") == 60 and COCO_LABELS.index("teddy bear") == 77


# ------------------------------------------------------------------------------------------- C ABI
def _built():
    if not os.path.exists(_lib.LIB_PATH):
        from layoutllm_t2i_amd.csrc.build import build
        build(verbose=False)
    return _lib.lib()


def test_layout_reward_entries_are_exported_under_abi_15():
    l = _built()
    assert hasattr(l, "gl_layout_reward") and hasattr(l, "gl_sizeof_layout_reward_args")
    assert l.gl_sizeof_layout_reward_args() == ctypes.sizeof(_lib.LayoutRewardArgs) == 88
    assert l.gl_abi_version() == _lib.ABI_VERSION == 15
    assert "gl_layout_reward" in _lib.PROTOTYPES and "gl_sizeof_layout_reward_args" in _lib.PROTOTYPES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gligen_hip.h")).read()
    assert "#define GL_LAYOUT_MAX_BOXES 64" in hdr and reward.MAX_BOXES == 64


def test_layout_reward_refuses_bad_arguments_before_any_launch():
    """every refusal is decided on the host from the args and the HOST count arrays: nothing is launched, so this runs without a GPU
    (the pointers named `device` are never read)"""
    l = _built()
    B = 3
    dev = (ctypes.c_double * 8)()                       # stands for device memory: refusals never dereference it
    n_gt, n_pred = (ctypes.c_int32 * B)(2, 1, 64), (ctypes.c_int32 * B)(0, 64, 3)

    def args(**kw):
        a = _lib.LayoutRewardArgs()
        p = ctypes.addressof(dev)
        a.boxes_gt = a.boxes_pred = a.labels_gt = a.labels_pred = a.n_gt = a.n_pred = a.miou = a.docsim = p
        a.n_gt_host, a.n_pred_host, a.B = ctypes.addressof(n_gt), ctypes.addressof(n_pred), B
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert l.gl_layout_reward(None, None) == -1 and "null args" in _lib.last_error(None)
    for field in ("boxes_gt", "boxes_pred", "labels_gt", "labels_pred", "n_gt", "n_pred", "n_gt_host", "n_pred_host", "miou", "docsim"):
        assert l.gl_layout_reward(ctypes.byref(args(**{field: None})), None) == -1, field
        assert _lib.last_error(None).startswith("gl_layout_reward:") and "null" in _lib.last_error(None), field
    for bad in (0, -4):
        assert l.gl_layout_reward(ctypes.byref(args(B=bad)), None) == -1 and f"B = {bad}" in _lib.last_error(None)
    for arr, name in ((n_gt, "n_gt"), (n_pred, "n_pred")):
        keep = arr[1]
        for bad in (65, -1):
            arr[1] = bad
            assert l.gl_layout_reward(ctypes.byref(args()), None) == -1
            assert f"{name}[1] = {bad} outside [0, 64]" in _lib.last_error(None)
        arr[1] = keep
    n_gt[2] = 0
    assert l.gl_layout_reward(ctypes.byref(args()), None) == -1 and "n_gt[2] = 0" in _lib.last_error(None)
    # the message is the calling thread's, a handle's message is its own
    buf = ctypes.create_string_buffer(8)
    assert l.gl_last_error(None, buf, 8) > 8 and buf.value == b"gl_layo"
    assert l.gl_last_error(None, None, 8) == -1
