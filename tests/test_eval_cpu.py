"""The depth evaluation suite's definition (tests/eval_ref.py) pinned on hand-worked cases, the host arithmetic of
codon_amd.metrics.depth_report, the command lines' refusals, and the conditions that keep tests/test_gpu_eval.py from passing
vacuously on the generator's cases.  No GPU."""
import math

import numpy as np
import pytest

from tests import eval_ref as E

# 3 x 3, T = 20: a step next to a hole -- (1,2) = 50 has the hole on its left and the 10 below it -- and steps on the border
L3 = np.array([[10, 10, 50],
               [10, 0, 50],
               [10, 10, 10]], dtype=np.uint8)
O3 = np.array([[12, 10, 28],
               [10, 7, 0],
               [9, 10, 14]], dtype=np.uint8)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_hand_worked_3x3(dtype):
    L, O = L3.astype(dtype), O3.astype(dtype)
    w, err, reg = E.depth_errors(L, O, thresholds=(0, 1, 3, 5), edge_threshold=20, edge_radius=0)
    # e = [[2, 0, 22], [0, -, 50], [1, 0, 4]] over the 8 valid pixels
    assert w.dtype == np.uint64 and w.tolist()[:4] == [8, 79, 4 + 484 + 2500 + 1 + 16, 50]
    assert w.tolist()[4:8] == [5, 4, 3, 2]
    # delta1: 10/12, 10/10 x3, 10/9;  delta2 adds 10/14 (16*14 < 25*10);  delta3 adds 50/28 (64*50 < 125*28);  50/0 never
    assert w.tolist()[8:11] == [5, 6, 7]
    # discontinuities: (0,1)|(0,2), (1,2)|(2,2); (1,0) and (2,1) only touch the hole
    assert w.tolist()[11:] == [4, 0 + 22 + 50 + 4, 484 + 2500 + 16, 0, 0]
    assert reg.dtype == np.uint8 and reg.tolist() == [[1, 2, 2], [1, 0, 2], [1, 1, 2]]
    assert err.dtype == dtype and err.tolist() == [[2, 0, 22], [0, 0, 50], [1, 0, 4]]
    # r = 1: everything valid but (2,0), which is two rows from (0,1) and two columns from (2,2)
    w1, _, reg1 = E.depth_errors(L, O, thresholds=(0, 1, 3, 5), edge_threshold=20, edge_radius=1)
    assert w1.tolist()[:11] == w.tolist()[:11] and w1.tolist()[11:14] == [7, 78, 3004]
    assert reg1.tolist() == [[2, 2, 2], [2, 0, 2], [1, 2, 2]]
    # a threshold at the step's size: |50 - 10| = 40 is not MORE than 40
    assert E.depth_errors(L, O, edge_threshold=40, edge_radius=8)[0].tolist()[11:14] == [0, 0, 0]
    assert E.depth_errors(L, O, edge_threshold=39, edge_radius=0)[0].tolist()[11] == 4
    # edge evaluation off, fewer thresholds
    w0, _, reg0 = E.depth_errors(L, O, thresholds=(3,))
    assert w0.tolist() == [8, 79, 3005, 50, 3, 0, 0, 0, 5, 6, 7, 0, 0, 0, 0, 0] and reg0.tolist() == [[1, 1, 1], [1, 0, 1], [1, 1, 1]]


def test_hand_worked_5x7_window_and_border():
    """A 6 x 9 label for a 5 x 7 output: the label's row 5 and columns 7, 8 hold a step that lies BEYOND the window and must
    not make row 4 or column 6 discontinuities; the only step inside is the corner pixel, and its dilation by r = 2 is cut by
    the image's border."""
    L = np.full((6, 9), 100, dtype=np.uint16)
    L[5, :], L[:, 7:] = 200, 200
    L[0, 0], L[2, 2] = 200, 0
    O = np.full((5, 7), 100, dtype=np.uint16)
    O[0, 0], O[2, 2], O[4, 6], O[1, 1] = 190, 5, 103, 97
    w, err, reg = E.depth_errors(L, O, thresholds=(2,), edge_threshold=50, edge_radius=0)
    assert w.tolist() == [34, 16, 118, 10, 3, 0, 0, 0, 34, 34, 34, 3, 10, 100, 0, 0]
    assert sorted(zip(*np.nonzero(reg == 2))) == [(0, 0), (0, 1), (1, 0)]
    w2, _, reg2 = E.depth_errors(L, O, thresholds=(2,), edge_threshold=50, edge_radius=2)
    # rows 0-2 x columns 0-3 and row 3 x columns 0-2, less the hole at (2,2)
    assert w2.tolist()[11:14] == [14, 13, 109]
    want = np.ones((5, 7), dtype=np.uint8)
    want[:3, :4], want[3, :3], want[2, 2] = 2, 2, 0
    assert np.array_equal(reg2, want)
    assert err[0, 0] == 10 and err[2, 2] == 0 and err[4, 6] == 3 and int(err.sum()) == 16
    w8 = E.depth_errors(L, O, edge_threshold=50, edge_radius=8)[0]
    assert w8.tolist()[11:14] == w8.tolist()[:3]                   # r = 8 covers the whole window


def test_all_holes_and_no_discontinuity():
    Z = np.zeros((4, 6), dtype=np.uint8)
    w, err, reg = E.depth_errors(Z, np.full((4, 6), 9, dtype=np.uint8), thresholds=(0, 1), edge_threshold=0, edge_radius=3)
    assert w.tolist() == [0] * 16 and not err.any() and not reg.any()
    with pytest.raises(ZeroDivisionError):
        E.depth_report(w)
    flat = np.full((4, 6), 7, dtype=np.uint8)
    r = E.depth_report(E.depth_errors(flat, flat + 1, edge_threshold=0, edge_radius=8)[0])
    assert r["edge_fraction"] == 0.0 and math.isnan(r["edge_mad"]) and math.isnan(r["edge_rmse"])
    assert r["flat_mad"] == r["mad"] == 1.0 and r["flat_rmse"] == r["rmse"] == 1.0
    full = E.depth_report(E.depth_errors(L3, O3, edge_threshold=0, edge_radius=8)[0])
    assert full["edge_fraction"] == 1.0 and math.isnan(full["flat_mad"]) and math.isnan(full["flat_rmse"])


@pytest.mark.parametrize("bits", [8, 16])
def test_rmse_equals_the_float64_loop_and_flat_is_all_minus_edge(bits):
    label, out = E.case((1, 33, 70), bits)
    L, O = label[0], out[0]
    w, err, reg = E.depth_errors(L, O, edge_radius=1, **E.PARAMS[bits])
    s, c = 0.0, 0                                                  # masked_rmse's definition: the reference's float64 loop
    for l, o in zip(L[:33, :70].ravel().tolist(), O.ravel().tolist()):
        if l != 0:
            s += (float(l) - float(o)) ** 2
            c += 1
    r = E.depth_report(w, thresholds=E.PARAMS[bits]["thresholds"])
    assert r["rmse"] == math.sqrt(s / c) and r["n"] == c
    e = err.astype(np.int64)
    for name, m in (("edge", reg == 2), ("flat", reg == 1)):
        assert r[name + "_mad"] == int(e[m].sum()) / int(m.sum())
        assert r[name + "_rmse"] == math.sqrt(int((e[m] ** 2).sum()) / int(m.sum()))
    assert int(w[0]) - int(w[11]) == int((reg == 1).sum()) and int(w[1]) - int(w[12]) == int(e[reg == 1].sum())


def test_depth_report_is_the_restatements_arithmetic():
    from codon_amd import metrics
    for bits in (8, 16):
        label, out = E.case((3, 37, 53), bits)
        thr = E.PARAMS[bits]["thresholds"]
        for w in E.depth_errors_batch(label, out, edge_radius=3, **E.PARAMS[bits])[0]:
            got, want = metrics.depth_report(w, unit=0.1, thresholds=thr), E.depth_report(w, unit=0.1, thresholds=thr)
            assert got == want and list(got) == list(want)
            assert list(got) == ["n", "mad", "rmse", "max"] + [f"bad>{t}" for t in thr] + [
                "delta1", "delta2", "delta3", "edge_fraction", "edge_mad", "edge_rmse", "flat_mad", "flat_rmse"]
            assert metrics.depth_report(w)["rmse"] == math.sqrt(int(w[2]) / int(w[0]))
    nan = metrics.depth_report([5, 5, 5, 1, 0, 0, 0, 0, 5, 5, 5, 0, 0, 0, 0, 0])
    assert math.isnan(nan["edge_mad"]) and math.isnan(nan["edge_rmse"]) and nan["flat_mad"] == 1.0
    with pytest.raises(ZeroDivisionError):
        metrics.depth_report([0] * 16)
    with pytest.raises(ValueError):
        metrics.depth_report([1] * 15)
    a, b = dict(nan), metrics.depth_report([4, 8, 16, 2, 0, 0, 0, 0, 4, 4, 4, 2, 6, 10, 0, 0])
    m = metrics.report_means([{"file": "a.png", **a}, {"file": "b.png", **b}])      # as the loop keeps them
    assert m == metrics.report_means([a, b])
    assert m["mad"] == [(1.0 + 2.0) / 2, 2] and m["edge_mad"] == [3.0, 1] and "n" not in m
    assert metrics.report_tokens(m).startswith("mad=1.5/2 ") and "edge_mad=3.0/1" in metrics.report_tokens(m)
    assert metrics.report_tokens(b).split()[:3] == ["n=4", "mad=2.0", "rmse=2.0"]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shape", [(1, 33, 70), (3, 37, 53)])
def test_generator_cases_are_not_vacuous(shape, bits):
    label, out = E.case(shape, bits)
    B, H, W = shape
    assert label.shape == (B, H + 3, W + 5) and out.shape == shape and label.dtype == out.dtype == E.DTYPE[bits]
    assert np.array_equal(label, E.case(shape, bits)[0])           # deterministic
    for r in (0, 1, 3):
        words, err, reg = E.depth_errors_batch(label, out, edge_radius=r, **E.PARAMS[bits])
        for b in range(B):
            w = [int(v) for v in words[b]]
            n = w[0]
            assert (label[b, :H, :W] == 0).any() and 0 < n < H * W
            assert 0 < w[11] < n
            assert all(0 < w[4 + k] < n for k in (1, 2, 3)) and w[4] > w[5] > w[6] > w[7]
            assert 0 < w[8] < w[9] < w[10] < n
            assert (reg[b] == 1).any() and (reg[b] == 2).any() and (reg[b] == 0).any()
            assert w[3] > 0 and err[b].max() == w[3]
    # the label's extra rows and columns matter: cropping by the wrong stride would change the words
    assert not np.array_equal(label[:, :H, :W], label[:, 3:, 5:])


def test_report_json_is_strict(tmp_path):
    """nan -- a value over an empty set -- is written as null: a strict parser reads the file."""
    import json
    from codon_amd import infer, metrics
    reps = [{"file": "a.png", **metrics.depth_report([5, 5, 5, 1, 0, 0, 0, 0, 5, 5, 5, 0, 0, 0, 0, 0], thresholds=(0,))},
            {"file": "b.png", **metrics.depth_report([4, 8, 16, 2, 4, 0, 0, 0, 4, 4, 4, 4, 8, 16, 0, 0], thresholds=(0,))}]
    means = metrics.report_means(reps)
    assert math.isnan(reps[0]["edge_mad"]) and math.isnan(reps[1]["flat_rmse"]) and means["edge_mad"] == [2.0, 1]
    p = str(tmp_path / "r.json")
    infer.write_report_json(p, reps, means)

    def refuse(c):
        raise AssertionError(c)
    doc = json.loads(open(p).read(), parse_constant=refuse)
    assert doc["images"][0]["edge_mad"] is None and doc["images"][0]["flat_mad"] == 1.0 and doc["images"][0]["file"] == "a.png"
    assert doc["images"][1]["flat_rmse"] is None and doc["images"][1]["edge_rmse"] == 2.0 and doc["images"][1]["bad>0"] == 1.0
    assert doc["means"]["edge_mad"] == [2.0, 1] and doc["means"]["mad"] == [1.5, 2]
    infer.write_report_json(p, reps[:1], metrics.report_means(reps[:1]))
    assert json.loads(open(p).read(), parse_constant=refuse)["means"]["edge_mad"] == [None, 0]


def test_cli_refusals(capsys):
    from codon_amd import infer, train
    base = ["--input-depth", "d", "--input-color", "c"]
    for extra, msg in ((["--report"], "--report needs --label"),
                       (["--label", "l", "--bad-thresholds", "1,2"], "--bad-thresholds needs --report"),
                       (["--label", "l", "--edge-threshold", "3"], "--edge-threshold needs --report"),
                       (["--label", "l", "--edge-radius", "3"], "--edge-radius needs --report"),
                       (["--label", "l", "--report-json", "x.json"], "--report-json needs --report"),
                       (["--label", "l", "--error-maps", "x"], "--error-maps needs --report"),
                       (["--label", "l", "--report", "--bad-thresholds", "1,2,3,4,5"], "at most 4"),
                       (["--label", "l", "--report", "--bad-thresholds", "1,-2"], "none negative"),
                       (["--label", "l", "--report", "--bad-thresholds", "1,x"], "integers in codes"),
                       (["--label", "l", "--report", "--edge-threshold", "-1"], "must not be negative"),
                       (["--label", "l", "--report", "--edge-radius", "2"], "--edge-radius needs --edge-threshold"),
                       (["--label", "l", "--report", "--edge-threshold", "5", "--edge-radius", "9"], "must lie in [0, 8]")):
        with pytest.raises(SystemExit) as e:
            infer.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    tbase = ["--scale", "4", "--train-depth", "d", "--train-color", "c", "--val-depth", "d", "--val-color", "c"]
    for extra, msg in ((["--val-report"], "--val-report needs --val-label"),
                       (["--val-label", "l", "--val-edge-threshold", "3"], "--val-edge-threshold needs --val-report"),
                       (["--val-label", "l", "--val-report", "--val-edge-threshold", "3", "--val-edge-radius", "11"], "must lie in [0, 8]")):
        with pytest.raises(SystemExit) as e:
            train.parse_args(tbase + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    a = train.parse_args(tbase + ["--val-label", "l", "--val-report", "--val-bad-thresholds", "1,3", "--val-edge-threshold", "20"])
    assert a.val_report is True and a.val_report_params == {"thresholds": (1, 3), "edge_threshold": 20, "edge_radius": 1}
    assert train.parse_args(tbase).val_report_params is None
