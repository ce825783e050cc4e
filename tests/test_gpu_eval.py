"""The depth evaluation suite on the GPU (codon_amd/csrc/eval.hip, codon_amd.metrics.depth_errors / depth_report, the --report
flags of codon_amd.infer and --val-report of codon_amd.train) against the numpy restatement tests/eval_ref.py:
equal bits throughout, on u8 and u16 codes."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import eval_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

_cache = {}


def _case(shape, bits):
    """(label, out) numpy planes and their device tensors (u16 as torch.uint16), built once and never written to."""
    k = (shape, bits)
    if k not in _cache:
        label, out = E.case(shape, bits)
        _cache[k] = (label, out, torch.from_numpy(label).to(DEV), torch.from_numpy(out).to(DEV))
    return _cache[k]


def _ref(shape, bits, **kw):
    k = (shape, bits, tuple(sorted(kw.items())))
    if k not in _cache:
        label, out = _case(shape, bits)[:2]
        _cache[k] = E.depth_errors_batch(label, out, **kw)
    return _cache[k]


def _words(acc):
    assert acc.dtype == torch.int64 and acc.is_cuda
    return acc.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("r", E.RADII)
@pytest.mark.parametrize("shape", E.SHAPES)
def test_words_and_maps_equal_bits(shape, r, bits):
    from codon_amd import metrics
    _, _, label, out = _case(shape, bits)
    kw = dict(E.PARAMS[bits], edge_radius=r)
    words, err, reg = _ref(shape, bits, **kw)
    acc, gerr, greg = metrics.depth_errors(label, out, error_map=True, region_map=True, **kw)
    assert acc.shape == (shape[0], 16) and np.array_equal(_words(acc), words), (_words(acc), words)
    assert gerr.dtype == out.dtype and gerr.shape == out.shape and np.array_equal(gerr.cpu().numpy(), err)
    assert greg.dtype == torch.uint8 and greg.shape == out.shape and np.array_equal(greg.cpu().numpy(), reg)
    # the maps are optional, one at a time, and do not change the words; a second call gives the same words
    only = metrics.depth_errors(label, out, **kw)
    assert torch.is_tensor(only) and torch.equal(only, acc)
    a2, r2 = metrics.depth_errors(label, out, region_map=True, **kw)
    assert torch.equal(a2, acc) and torch.equal(r2, greg)
    # an image alone, as (H, W) planes cut out of the batch (a strided label): its own row of words, (H, W) maps
    b = shape[0] - 1
    a1, e1 = metrics.depth_errors(label[b], out[b], error_map=True, **kw)
    assert a1.shape == (1, 16) and np.array_equal(_words(a1)[0], words[b]) and np.array_equal(e1.cpu().numpy(), err[b])
    # a window of the label, not contiguous: its strides reach the kernel (the columns cut off lie beyond the output's anyway)
    cut = label[:, :shape[1] + 1, :shape[2] + 2]
    assert not cut.is_contiguous() and torch.equal(metrics.depth_errors(cut, out, **kw), acc)
    # one label for every image of the batch (image stride 0): copied first, then the same as the label repeated
    if shape[0] > 1:
        lv = label.view(torch.int16) if bits == 16 else label
        one = metrics.depth_errors(lv[:1].expand(shape[0], -1, -1), out, **kw)
        assert torch.equal(one, metrics.depth_errors(lv[:1].repeat(shape[0], 1, 1), out, **kw)) and torch.equal(one[0], acc[0])


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("shape", E.SHAPES)
def test_edge_off_and_fewer_thresholds(shape, bits):
    from codon_amd import metrics
    _, _, label, out = _case(shape, bits)
    thr = E.PARAMS[bits]["thresholds"][1:3]
    words, err, reg = _ref(shape, bits, thresholds=thr)
    acc, gerr, greg = metrics.depth_errors(label, out, thresholds=thr, error_map=True, region_map=True)
    got = _words(acc)
    assert np.array_equal(got, words) and np.array_equal(gerr.cpu().numpy(), err) and np.array_equal(greg.cpu().numpy(), reg)
    assert not got[:, 6:8].any() and not got[:, 11:].any() and got[:, 4:6].all() and set(np.unique(reg)) == {0, 1}
    none = _words(metrics.depth_errors(label, out))
    assert np.array_equal(none[:, :4], words[:, :4]) and not none[:, 4:8].any() and np.array_equal(none[:, 8:11], words[:, 8:11])


@pytest.mark.parametrize("bits", [8, 16])
def test_all_hole_image_and_carriers(bits):
    from codon_amd import metrics
    shape = (3, 37, 53)
    label, out, dl, do = _case(shape, bits)
    kw = dict(E.PARAMS[bits], edge_radius=3)
    holes = dl.view(torch.int16).clone() if bits == 16 else dl.clone()
    holes[1] = 0                                                           # the middle image: every label pixel a hole
    acc, gerr, greg = metrics.depth_errors(holes, do, error_map=True, region_map=True, **kw)
    want = _ref(shape, bits, **kw)[0].copy()
    want[1] = 0
    assert np.array_equal(_words(acc), want) and not gerr[1].view(torch.uint8).any() and not greg[1].any()
    if bits == 16:                                                         # the same bits held as int16: equal results
        words = _ref(shape, bits, **kw)
        li, oi = dl.view(torch.int16), do.view(torch.int16)
        for a, b in ((li, oi), (li, do), (dl, oi)):
            acc, gerr = metrics.depth_errors(a, b, error_map=True, **kw)
            assert np.array_equal(_words(acc), words[0]) and gerr.dtype == b.dtype
            assert np.array_equal(gerr.view(torch.uint16).cpu().numpy(), words[1])


@pytest.mark.parametrize("shape", [(1, 33, 70), (3, 37, 53)])
def test_report_rmse_is_masked_rmse(shape):
    from codon_amd import metrics
    for bits, rmse in ((8, metrics.masked_rmse), (16, metrics.masked_rmse_u16)):
        _, _, label, out = _case(shape, bits)
        rows = metrics.depth_errors(label, out, **E.PARAMS[bits]).cpu()
        for b in range(shape[0]):
            rep = metrics.depth_report(rows[b], thresholds=E.PARAMS[bits]["thresholds"])
            assert rep["rmse"] == rmse(label[b], out[b])
            assert rep == E.depth_report(_ref(shape, bits, edge_radius=1, **E.PARAMS[bits])[0][b], thresholds=E.PARAMS[bits]["thresholds"])


def test_refusals():
    from codon_amd import metrics
    _, _, label, out = _case((1, 33, 70), 8)
    for kw, msg in (({"edge_threshold": 20, "edge_radius": 9}, "edge_radius 9"),
                    ({"edge_threshold": 20, "edge_radius": -1}, "edge_radius -1"),
                    ({"thresholds": (0, 1, 2, 3, 4)}, "5 thresholds"),
                    ({"thresholds": (1, -1)}, "negative"),
                    ({"edge_threshold": -1}, "negative")):
        with pytest.raises(RuntimeError, match=msg):
            metrics.depth_errors(label, out, **kw)
    with pytest.raises(RuntimeError, match="smaller than the 33x70 output"):
        metrics.depth_errors(label[:, :32], out)
    with pytest.raises(RuntimeError, match="smaller than the 33x70 output"):
        metrics.depth_errors(label[:, :, :69], out)
    with pytest.raises(ValueError):
        metrics.depth_errors(label, _case((1, 33, 70), 16)[3])
    with pytest.raises(ValueError):
        metrics.depth_errors(label, out, thresholds=(1.5,))


# ---- the command lines -----------------------------------------------------------------------------------------------------------

SIZES = [(24, 40), (24, 40), (21, 37)]
FLAGS = ["--report", "--bad-thresholds", "1,3,8", "--edge-threshold", "20", "--edge-radius", "2"]
REPORT = {"thresholds": (1, 3, 8), "edge_threshold": 20, "edge_radius": 2}


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """Three tiny synthetic pairs as 8-bit PNGs -- depth, guidance, and a label 3 rows and 5 columns larger with steps and holes --
    and a checkpoint of randomly initialised weights."""
    from codon_amd import CODONNet, io
    root = tmp_path_factory.mktemp("eval_pairs")
    dirs = [str(root / n) for n in ("depth", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    g = np.random.default_rng(11)
    labels = {}
    for i, (h, w) in enumerate(SIZES):
        label = E.case((1, h, w), 8, seed=100 + i)[0][0]
        name = f"{i:02d}.png"
        io.write_gray(os.path.join(dirs[0], name), np.where(label[:h, :w] == 0, 128, label[:h, :w]).astype(np.uint8))
        io.write_gray(os.path.join(dirs[1], name), g.integers(0, 256, size=(h, w), dtype=np.uint8))
        io.write_gray(os.path.join(dirs[2], name), label)
        labels[name] = label
    torch.manual_seed(5)
    ck = str(root / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    return dirs, labels, ck, root


def test_infer_report_serial_pipeline_and_values(pairs, capsys):
    from codon_amd import infer, io, metrics
    (dd, cd, ld), labels, ck, root = pairs
    base = ["--input-depth", dd, "--input-color", cd, "--label", ld, "--weights", ck, "--dtype", "f32"]
    runs = {}
    for mode in ("serial", "pipe"):
        od, ed, js = (str(root / f"{n}_{mode}") for n in ("out", "err", "json"))
        capsys.readouterr()
        assert infer.main(base + FLAGS + ["--out", od, "--error-maps", ed, "--report-json", js] +
                          (["--serial"] if mode == "serial" else [])) == 0
        runs[mode] = (capsys.readouterr().out, {n: open(os.path.join(ed, n), "rb").read() for n in labels}, open(js).read(),
                      {n: open(os.path.join(od, n), "rb").read() for n in labels})
    assert runs["serial"] == runs["pipe"]
    text, _, js, _ = runs["pipe"]
    lines = text.splitlines()
    assert len(lines) == 1 + 3 + 2 + 1
    reports = []
    for ln, (name, label) in zip(lines[1:4], sorted(labels.items())):
        out = io.read_gray(str(root / "out_pipe" / name))
        words, err, _ = E.depth_errors(label, out, **REPORT)
        rep = E.depth_report(words, thresholds=REPORT["thresholds"])
        f, rm, ss, rest = ln.split(" ", 3)
        assert f == name and float(rm) == rep["rmse"] and rest == metrics.report_tokens(rep)
        assert f"bad>3={rep['bad>3']!r}" in rest.split() and f"edge_rmse={rep['edge_rmse']!r}" in rest.split()
        assert 0 < rep["edge_fraction"] < 1
        emap = io.read_gray(str(root / "err_pipe" / name))
        assert emap.dtype == np.uint8 and np.array_equal(emap, err)
        reports.append({"file": name, **rep})
    means = metrics.report_means(reports)
    assert means["rmse"] == [sum(r["rmse"] for r in reports) / 3, 3] and float(lines[5].split()[0]) == means["rmse"][0]
    assert lines[6] == "mean " + metrics.report_tokens(means) and f"mad={means['mad'][0]!r}/3" in lines[6].split()
    assert json.loads(js) == json.loads(json.dumps({"images": reports, "means": means}))
    # without --report: today's lines -- the same first three tokens and nothing more, no means line, no file
    capsys.readouterr()
    assert infer.main(base + ["--out", str(root / "out_plain")]) == 0
    plain = capsys.readouterr().out.splitlines()
    assert plain == [lines[0]] + [" ".join(ln.split()[:3]) for ln in lines[1:4]] + lines[4:6]
    assert all(open(root / "out_plain" / n, "rb").read() == b for n, b in runs["pipe"][3].items())


def test_infer_report_16bit_unit_error_maps_and_null(tmp_path, capsys):
    """--depth-bits 16 --depth-unit 0.1 --report --error-maps without --edge-threshold: mad, rmse and max are in codes times the
    unit, the error maps are 16-bit PNGs, the label travels as u16 bits, and the edge values -- nan -- are null in the JSON."""
    from codon_amd import CODONNet, infer, io, metrics
    dirs = [str(tmp_path / n) for n in ("depth", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    g = np.random.default_rng(12)
    labels = {}
    for i, (h, w) in enumerate(SIZES[1:]):
        label = E.case((1, h, w), 16, seed=200 + i)[0][0]
        name = f"{i:02d}.png"
        io.write_depth16(os.path.join(dirs[0], name), np.where(label[:h, :w] == 0, 30000, label[:h, :w]).astype(np.uint16))
        io.write_gray(os.path.join(dirs[1], name), g.integers(0, 256, size=(h, w), dtype=np.uint8))
        io.write_depth16(os.path.join(dirs[2], name), label)
        labels[name] = label
    torch.manual_seed(6)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 1, "model": CODONNet()}, ck)
    thr, unit = (200, 1000), 0.1
    runs = {}
    for mode in ("serial", "pipe"):
        od, ed, js = (str(tmp_path / f"{n}_{mode}") for n in ("out", "err", "json"))
        capsys.readouterr()
        assert infer.main(["--input-depth", dirs[0], "--input-color", dirs[1], "--label", dirs[2], "--weights", ck, "--dtype", "f32",
                           "--depth-bits", "16", "--depth-unit", str(unit), "--report", "--bad-thresholds", "200,1000",
                           "--out", od, "--error-maps", ed, "--report-json", js] + (["--serial"] if mode == "serial" else [])) == 0
        runs[mode] = (capsys.readouterr().out, {n: open(os.path.join(ed, n), "rb").read() for n in labels}, open(js).read())
    assert runs["serial"] == runs["pipe"]
    lines = runs["pipe"][0].splitlines()
    assert len(lines) == 1 + 2 + 2 + 1

    def refuse(c):
        raise AssertionError(f"{c} in the JSON report")
    doc = json.loads(runs["pipe"][2], parse_constant=refuse)
    for k, (ln, (name, label)) in enumerate(zip(lines[1:3], sorted(labels.items()))):
        out = io.read_depth(str(tmp_path / "out_pipe" / name))
        assert out.dtype == np.uint16
        words, err, _ = E.depth_errors(label, out, thresholds=thr)
        rep = E.depth_report(words, unit=unit, thresholds=thr)
        f, rm, ss, rest = ln.split(" ", 3)
        assert f == name and float(rm) == rep["rmse"] == math.sqrt(int(words[2]) / int(words[0])) * unit
        assert rest == metrics.report_tokens(rep) and "edge_mad=nan" in rest.split() and f"max={int(words[3]) * unit!r}" in rest.split()
        assert rep["mad"] == int(words[1]) / int(words[0]) * unit and rep["bad>200"] == int(words[4]) / int(words[0])
        emap = io.read_depth(str(tmp_path / "err_pipe" / name))
        assert emap.dtype == np.uint16 and np.array_equal(emap, err) and int(emap.max()) > 255
        img = doc["images"][k]
        assert img["file"] == name and img["rmse"] == rep["rmse"] and img["edge_fraction"] == 0.0
        assert img["edge_mad"] is None and img["edge_rmse"] is None and img["flat_mad"] == rep["flat_mad"] == rep["mad"]
    assert doc["means"]["edge_mad"] == [None, 0] and doc["means"]["rmse"][1] == 2
    assert lines[5].startswith("mean mad=") and "edge_mad=nan/0" in lines[5].split()


def _call_log():
    spec = importlib.util.spec_from_file_location("abi_call_log", os.path.join(ROOT, "tools", "abi_call_log.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_run_issues_the_same_calls(pairs):
    """The ABI call log of the loop with the report is the log of the loop without it plus one codon_depth_errors per image."""
    from codon_amd import CODONNet, infer
    from codon_amd import _lib as L
    (dd, cd, ld), labels, _, _ = pairs
    model = CODONNet().to(DEV).eval()
    acl, logs, bound = _call_log(), {}, L.load()
    infer.run_loop(model, torch.device(DEV), torch.float32, dd, cd, ld, pipelined=False, emit=lambda s: None)   # packs the weights
    try:
        for pipelined in (False, True):
            for rp in (None, REPORT):
                log = acl.install()
                infer.run_loop(model, torch.device(DEV), torch.float32, dd, cd, ld, pipelined=pipelined, emit=lambda s: None,
                               **({"report": rp} if rp else {}))
                logs[pipelined, rp is not None] = [c for c in log if c[0] != "codon_build_source_hash"]
    finally:
        L._lib = bound
    for pipelined in (False, True):
        plain, rep = logs[pipelined, False], logs[pipelined, True]
        extra = [c for c in rep if c[0] == "codon_depth_errors"]
        assert not any(c[0] == "codon_depth_errors" for c in plain) and len(extra) == len(labels)
        assert acl.diff(plain, [c for c in rep if c[0] != "codon_depth_errors"]) is None
        d = extra[0][1][0]
        assert (d["batch"], d["height"], d["width"], d["label_height"], d["label_row_stride"]) == (1, 24, 40, 27, 45)
        assert d["thresholds"][:3] == [1, 3, 8] and (d["edge"], d["edge_threshold"], d["edge_radius"]) == (1, 20, 2)


def test_validate_val_report(pairs):
    from codon_amd import CODONNet, infer, metrics, train
    (dd, cd, ld), _, _, _ = pairs
    torch.manual_seed(7)
    model = CODONNet().to(DEV)
    val = {"depth": dd, "color": cd, "label": ld}
    plain, lines = [], []
    train.validate(model, torch.device(DEV), val, emit=plain.append)
    r = train.validate(model, torch.device(DEV), dict(val, report=REPORT), emit=lines.append)
    assert model.training and len(plain) == 1 and len(lines) == 2 and lines[0] == plain[0] and lines[0].startswith("val 3 images rmse ")
    want = infer.run_loop(model.eval(), torch.device(DEV), torch.float32, dd, cd, ld, emit=lambda s: None, pipelined=False, report=REPORT)
    model.train()
    assert lines[1] == "val-report " + metrics.report_tokens(want["report_means"]) and r["report_means"] == want["report_means"]
    assert want["report_means"]["rmse"][0] == want["rmse_mean"] and not math.isnan(want["report_means"]["edge_mad"][0])
