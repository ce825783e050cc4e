"""What every codon_* entry that takes a dtype or a 16-bit channel slice REFUSES, and how: (return code, the text of
codon_last_error_string before its first ':').  tests/golden/c8_refusals.json is this table as recorded on the commit before the
16-bit host rules were stated once (python -m tests.c8_refusals OUT.json); tests/test_c8_refusals.py holds the
library to it.  Only codon_amd._lib names are used, so the module runs unchanged on an older tree.  Pointers are small fake
aligned integers and nothing is allocated: every case is refused before any HIP call, which the recording asserts (a call that
reached a launch without a device would return CODON_ERR_LAUNCH)."""
import ctypes as C
import json
import sys

from codon_amd import _lib as L

P, ODD = 0x10000, 0x10001                       # a fake 16-byte aligned device pointer, and a misaligned one
BIG128, BIG64 = (4096, 4100), (8192, 4100)      # H W * 2 bytes * 128 (64) channels passes the buffer-descriptor range
DESC = dict(batch=2, height=19, width=70, cin=64, cout=64, ksize=3, x_ctotal=72, x_coff=8, y_ctotal=72, y_coff=8,
            r_ctotal=72, r_coff=8, flags=0, dtype=L.BF16)
DESC_FIELDS = [f[0] for f in L.ConvDesc._fields_]


def _entry(name, args, **over):
    """args: (kind, name[, default]) with kind d = the conv descriptor, p = pointer, t = codon_tensor*, i = int."""
    return dict(name=name, args=args, base=over)


_BHW = [("i", "batch", 2), ("i", "height", 19), ("i", "width", 70)]
ENTRIES = {e["name"]: e for e in [
    _entry("codon_conv_pack_weight", [("p", "w"), ("p", "out"), ("i", "cout", 64), ("i", "cin", 64), ("i", "ksize", 3),
                                      ("i", "mode", 0), ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_conv2d_fwd", [("d",), ("p", "x"), ("p", "w"), ("p", "y"), ("p", "res"), ("p", "stream")]),
    _entry("codon_conv2d_sum_into_fwd", [("d",), ("p", "x"), ("p", "w"), ("p", "y"), ("p", "sum", P + 0x100), ("p", "stream")],
           ksize=5),
    _entry("codon_conv_chain1x1_fwd", [("d",), ("p", "x"), ("p", "w"), ("p", "y"), ("p", "w_chain"), ("t", "out"), ("t", "res"),
                                       ("p", "stream")], ksize=5, cin=128, cout=128, x_ctotal=136, y_ctotal=136, flags=1),
    _entry("codon_conv_chain1x1_stats_fwd", [("d",), ("p", "x"), ("p", "w"), ("p", "y"), ("p", "w_chain"), ("t", "out"),
                                             ("t", "res"), ("p", "pool"), ("p", "partials"), ("i", "choff", 64), ("p", "stream")],
           ksize=5, cin=128, cout=128, x_ctotal=136, y_ctotal=136, flags=1),
    _entry("codon_conv2d_gated_fwd", [("d",), ("p", "pre"), ("t", "inputs"), ("p", "ch"), ("p", "sp"), ("p", "w"), ("p", "y"),
                                      ("p", "stream")], x_coff=0),
    _entry("codon_conv2d_gated_emit_fwd", [("d",), ("p", "pre"), ("t", "inputs"), ("p", "ch"), ("p", "sp"), ("p", "w"), ("p", "y"),
                                           ("t", "gated_out"), ("p", "stream")], x_coff=0),
    _entry("codon_conv2d_wgrad", [("d",), ("p", "x"), ("p", "gy"), ("p", "dw"), ("p", "ws"), ("i", "ws_bytes", 0),
                                  ("i", "accumulate", 0), ("p", "stream")]),
    _entry("codon_conv1x1_bwd", [("d",), ("p", "x"), ("p", "gy"), ("p", "w"), ("t", "gx", (136, 8)), ("p", "dw"), ("p", "ws"),
                                 ("i", "ws_bytes", 0), ("i", "accumulate", 0), ("p", "stream")],
           ksize=1, cin=128, x_ctotal=136),
    _entry("codon_conv1x1_bwd_gated", [("d",), ("p", "x"), ("p", "gy"), ("p", "w"), ("t", "gx", (136, 8)), ("p", "dw"), ("p", "ws"),
                                       ("i", "ws_bytes", 0), ("i", "accumulate", 0), ("p", "ch"), ("p", "sp"), ("p", "g_pooled"),
                                       ("p", "g_pools"), ("p", "argpix"), ("p", "argch"), ("i", "fcat_base", 64), ("p", "stream")],
           ksize=1, cin=128, x_ctotal=136),
    _entry("codon_conv_form_c8", [("d",)]),
    _entry("codon_stem_fwd", _BHW + [("p", "x"), ("p", "w"), ("p", "y"), ("i", "ctotal", 72), ("i", "coff", 8),
                                     ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_stem_fwd_guarded", _BHW + [("p", "x"), ("p", "w"), ("p", "y"), ("i", "ctotal", 72), ("i", "coff", 8),
                                             ("i", "dtype", L.BF16), ("p", "bad"), ("p", "host"), ("p", "stream")]),
    _entry("codon_stem_pair_fwd", _BHW + [("p", "x"), ("p", "w"), ("p", "y"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "xb"),
                                          ("p", "wb"), ("p", "yb", P + 0x100), ("i", "yb_ctotal", 72), ("i", "yb_coff", 8),
                                          ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_head_fwd", _BHW + [("p", "x"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "w"), ("p", "res"), ("p", "y"),
                                     ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_head_fwd_y16", _BHW + [("p", "x"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "w"), ("p", "res"), ("p", "y"),
                                         ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_cac_stats_fwd", _BHW + [("t", "pre_c"), ("t", "pre"), ("p", "pooled"), ("p", "partials"), ("i", "dtype", L.BF16),
                                          ("p", "stream")]),
    _entry("codon_cac_stats_scaled_fwd", _BHW + [("t", "pre_c"), ("t", "pre"), ("p", "ch"), ("p", "pooled"), ("p", "partials"),
                                                 ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_ew_sq_scale", _BHW + [("t", "x"), ("p", "ch"), ("t", "y"), ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_cac_apply_fwd", _BHW + [("t", "pre"), ("t", "pre_c"), ("p", "ch"), ("p", "sp"), ("t", "inputs"), ("t", "inputs_c"),
                                          ("t", "out"), ("t", "out_c"), ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_stencil_1to64", _BHW + [("p", "x"), ("p", "w"), ("t", "y"), ("i", "flags", 1), ("t", "mask"),
                                          ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_conv1ch_wgrad", _BHW + [("t", "a"), ("p", "s"), ("p", "dw"), ("i", "flip", 0), ("p", "ws"), ("i", "ws_bytes", 0),
                                          ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_ew_add_mask", _BHW + [("i", "channels", 64), ("t", "dst"), ("t", "src"), ("t", "mask"), ("i", "accumulate", 1),
                                        ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_ew_sum_mask", _BHW + [("i", "channels", 64), ("t", "dst"), ("i", "nsrc", 2), ("t", "src0", (72, 8, P + 0x100)),
                                        ("t", "src1", (72, 8, P + 0x200)), ("t", "src2", None), ("t", "src3", None), ("t", "mask"),
                                        ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_cac_bwd_reduce", _BHW + [("t", "g_out"), ("t", "g_out_c"), ("t", "pre"), ("t", "pre_c"), ("p", "ch"), ("p", "sp"),
                                           ("p", "pools"), ("p", "g_z"), ("p", "part_gch"), ("p", "part_arg"),
                                           ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_cac_bwd_reduce_acc", _BHW + [("t", "g_out"), ("t", "g_out_c"), ("t", "pre"), ("t", "pre_c"), ("p", "ch"),
                                               ("p", "sp"), ("p", "pools"), ("p", "pooled"), ("p", "g_z"), ("p", "part_gch"),
                                               ("p", "part_arg"), ("p", "argch"), ("t", "g_in"), ("t", "g_in_c"),
                                               ("i", "accumulate_in", 1), ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_cac_bwd_apply", _BHW + [("t", "g_out"), ("t", "g_out_c"), ("t", "pre"), ("t", "pre_c"), ("p", "ch"), ("p", "sp"),
                                          ("p", "pooled"), ("p", "g_pooled"), ("p", "g_pools"), ("p", "argpix"), ("t", "g_pre"),
                                          ("t", "g_pre_c"), ("t", "g_in"), ("t", "g_in_c"), ("i", "accumulate_in", 1),
                                          ("i", "dtype", L.BF16), ("p", "stream")]),
    _entry("codon_stem_pair_fwd_guarded", _BHW + [("p", "x"), ("p", "w"), ("p", "y"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "xb"),
                                                  ("p", "wb"), ("p", "yb", P + 0x100), ("i", "yb_ctotal", 72), ("i", "yb_coff", 8),
                                                  ("i", "dtype", L.BF16), ("p", "bad"), ("p", "host"), ("p", "host_b"), ("p", "stream")]),
    _entry("codon_head_fwd_guarded", _BHW + [("p", "x"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "w"), ("p", "res"), ("p", "y"),
                                             ("i", "dtype", L.BF16), ("p", "bad"), ("p", "stream")]),
    _entry("codon_head_fwd_y16_guarded", _BHW + [("p", "x"), ("i", "ctotal", 72), ("i", "coff", 8), ("p", "w"), ("p", "res"),
                                                 ("p", "y"), ("i", "dtype", L.BF16), ("p", "bad"), ("p", "stream")]),
    _entry("codon_lr_codes_to_input", _BHW + [("i", "scale", 4), ("p", "codes"), ("i", "code_bits", 16), ("p", "lut"),
                                              ("i", "depth_max", 65535), ("p", "phase_weights"), ("p", "out"), ("i", "dtype", L.BF16),
                                              ("p", "stream")]),
    _entry("codon_d4_views", _BHW + [("p", "src0"), ("p", "src1", None), ("i", "dtype", L.BF16), ("p", "upright0"),
                                     ("p", "transposed0"), ("p", "upright1", None), ("p", "transposed1", None), ("p", "stream")]),
    _entry("codon_d4_merge", _BHW + [("p", "upright"), ("p", "transposed"), ("i", "dtype", L.BF16), ("p", "out"), ("p", "stream")]),
    _entry("codon_cast_multi", [("c",), ("p", "dst"), ("p", "stream")]),
    _entry("codon_postprocess_u8_dt", [("i", "n", 100), ("p", "x"), ("i", "dtype", L.F16), ("p", "out"), ("p", "stream")]),
    _entry("codon_postprocess_u16_dt", [("i", "n", 100), ("p", "x"), ("i", "dtype", L.BF16), ("i", "depth_max", 65535), ("p", "out"),
                                        ("p", "stream")]),
]}


def call(name, over):
    """One call of entry `name` with its good arguments changed by `over`: desc fields / int arguments by name, pointers by name
    (None = null), tensors as "<name>" -> None / (ctotal, coff[, data]).  Returns (code, text before the first ':')."""
    e = ENTRIES[name]
    over = dict(e["base"], **over)
    args, keep, used = [], [], set()
    for a in e["args"]:
        kind, an = a[0], (a[1] if len(a) > 1 else None)
        if kind == "d":
            if over.get("desc", 1) is None:
                args.append(None); used.update(["desc"] + DESC_FIELDS)
                continue
            v = dict(DESC)
            for k in DESC_FIELDS:
                if k in over:
                    v[k] = over[k]; used.add(k)
            d = L.ConvDesc(*[v[k] for k in DESC_FIELDS])
            keep.append(d); args.append(C.byref(d))
        elif kind == "c":                                  # codon_cast_desc: two tensors, the second one's fields from `over`
            used.update(["n", "dtype", "src", "count"])
            if over.get("desc", 1) is None:
                args.append(None); used.add("desc")
                continue
            d = L.CastDesc()
            d.n = over.get("n", 2)
            d.src[0], d.count[0], d.dtype[0] = P, 16, L.F32
            d.src[1], d.count[1], d.dtype[1] = over.get("src", P), over.get("count", 16), over.get("dtype", L.BF16)
            keep.append(d); args.append(C.byref(d))
        elif kind == "p":
            used.add(an)
            args.append(over[an] if an in over else (None if an == "stream" else (a[2] if len(a) > 2 else P)))
        elif kind == "i":
            used.add(an)
            args.append(over.get(an, a[2]))
        else:
            used.add(an)
            v = over[an] if an in over else (a[2] if len(a) > 2 else (72, 8))
            if v is None:
                args.append(None)
                continue
            t = L.Tensor(v[2] if len(v) > 2 else P, v[0], v[1])
            keep.append(t); args.append(C.byref(t))
    assert set(over) <= used, (name, set(over) - used)
    lib = L.load()
    code = getattr(lib, name)(*args)
    return code, lib.codon_last_error_string().decode().split(":")[0]


def _uses(name, kind):
    return [a[1] for a in ENTRIES[name]["args"] if a[0] == kind]


FP32_TOO = {"codon_conv_pack_weight", "codon_conv2d_fwd", "codon_conv_chain1x1_fwd", "codon_conv_chain1x1_stats_fwd",
            "codon_conv2d_gated_fwd", "codon_conv2d_gated_emit_fwd", "codon_conv2d_wgrad", "codon_stem_fwd", "codon_stem_fwd_guarded",
            "codon_stem_pair_fwd", "codon_head_fwd", "codon_cac_stats_fwd", "codon_cac_stats_scaled_fwd", "codon_ew_sq_scale",
            "codon_cac_apply_fwd", "codon_stencil_1to64", "codon_conv1ch_wgrad", "codon_ew_add_mask", "codon_ew_sum_mask",
            "codon_cac_bwd_reduce", "codon_cac_bwd_apply", "codon_postprocess_u8_dt", "codon_postprocess_u16_dt",
            "codon_stem_pair_fwd_guarded", "codon_head_fwd_guarded", "codon_lr_codes_to_input", "codon_d4_views", "codon_d4_merge",
            "codon_cast_multi"}
NO_RANGE_CHECK = {"codon_ew_sq_scale", "codon_conv1ch_wgrad", "codon_conv_form_c8", "codon_conv_pack_weight",
                  "codon_postprocess_u8_dt", "codon_postprocess_u16_dt", "codon_conv2d_wgrad", "codon_conv1x1_bwd",
                  "codon_conv1x1_bwd_gated", "codon_lr_codes_to_input", "codon_d4_views", "codon_d4_merge", "codon_cast_multi"}          # no buffer-descriptor range refusal today (known: DESIGN 3.1.2)
SLICE_INTS = {"codon_stem_fwd": [("ctotal", "coff")], "codon_stem_fwd_guarded": [("ctotal", "coff")],
              "codon_stem_pair_fwd": [("ctotal", "coff"), ("yb_ctotal", "yb_coff")], "codon_head_fwd": [("ctotal", "coff")],
              "codon_head_fwd_y16": [("ctotal", "coff")], "codon_head_fwd_guarded": [("ctotal", "coff")],
              "codon_head_fwd_y16_guarded": [("ctotal", "coff")],
              "codon_stem_pair_fwd_guarded": [("ctotal", "coff"), ("yb_ctotal", "yb_coff")]}


def cases():
    """[(entry, case name, overrides)]: per entry the nulls, a bad shape, the dtypes, every slice out of bounds / off the
    8-channel planes, the image past the descriptor range, and by hand what is particular to an entry."""
    out = []
    for name, e in ENTRIES.items():
        desc = e["args"][0][0] == "d"
        if desc or name == "codon_cast_multi":
            out.append((name, "null_desc", dict(desc=None)))
        for p in _uses(name, "p"):
            if p not in ("stream", "res", "bad", "host", "host_b", "dw", "src1", "upright1", "transposed1") and not (p == "y" and "chain1x1" in name):
                out.append((name, f"null_{p}", {p: None}))
        for t in _uses(name, "t"):
            if t not in ("res", "mask", "src", "src2", "src3") and not (name == "codon_conv2d_gated_fwd" and t == "gated_out"):
                if (name, t) != ("codon_ew_sum_mask", "dst"):      # reads dst->data for the aliasing rule before it tests dst
                    out.append((name, f"null_{t}", {t: None}))
                out.append((name, f"null_data_{t}", {t: (72, 8, None)}))
        if name not in ("codon_conv_pack_weight", "codon_postprocess_u8_dt", "codon_postprocess_u16_dt", "codon_cast_multi"):
            out.append((name, "height_0", dict(height=0)))
            out.append((name, "batch_negative", dict(batch=-1)))
        out.append((name, "dtype_unknown", dict(dtype=7)))
        out.append((name, "dtype_negative", dict(dtype=-1)))
        if name not in FP32_TOO:
            out.append((name, "dtype_f32", dict(dtype=L.F32)))
        # slices: past the end (a whole plane count, so only the bounds rule is broken), then off the 8-channel planes
        slices = [(t, None) for t in _uses(name, "t") if t not in ("src2", "src3")] + [(None, s) for s in SLICE_INTS.get(name, [])]
        if desc and name != "codon_conv_form_c8":
            slices += [(None, ("x_ctotal", "x_coff")), (None, ("y_ctotal", "y_coff"))]
            if name in ("codon_conv2d_sum_into_fwd",):
                slices.append((None, ("r_ctotal", "r_coff")))
        for t, ints in slices:
            if name == "codon_conv2d_gated_fwd" and t == "gated_out":
                continue
            wide = 136 if (t == "gx" or (ints and ENTRIES[name]["base"].get(ints[0]) == 136)) else 72
            tag = t or ints[1]
            for cname, ct, co in (("past_end", wide, wide - 56), ("coff_negative", wide, -8), ("coff_4", wide + 8, 4),
                                  ("ctotal_76", wide + 4, 8)):
                if ints and ints[1] == "x_coff" and name.startswith("codon_conv2d_gated") and cname != "past_end":
                    continue                                  # the gated convs ask x_coff % 64 == 0 first: pinned by hand below
                out.append((name, f"{tag}_{cname}", {t: (ct, co)} if t else {ints[0]: ct, ints[1]: co}))
        if name not in NO_RANGE_CHECK:
            H, W = BIG128 if desc else BIG64
            out.append((name, "image_past_descriptor_range", dict(height=H, width=W)))
            out.append((name, "image_past_31_bits", dict(height=46341, width=46341)))
    by_hand = [
        ("codon_conv2d_fwd", "residual_flag_null_residual", dict(flags=L.CONV_ADD_RESIDUAL, res=None)),
        ("codon_conv2d_fwd", "residual_past_end", dict(flags=L.CONV_ADD_RESIDUAL, r_ctotal=72, r_coff=16)),
        ("codon_conv2d_fwd", "residual_coff_4", dict(flags=L.CONV_ADD_RESIDUAL, r_ctotal=80, r_coff=4)),
        ("codon_conv2d_fwd", "mask_coff_4", dict(flags=L.CONV_MASK_RELU, r_ctotal=80, r_coff=4)),
        ("codon_conv2d_fwd", "unknown_flag", dict(flags=1 << 16)),
        ("codon_conv2d_fwd", "residual_and_mask", dict(flags=L.CONV_ADD_RESIDUAL | L.CONV_MASK_RELU)),
        ("codon_conv2d_fwd", "mask_sum_alone", dict(flags=L.CONV_MASK_SUM)),
        ("codon_conv2d_fwd", "weights_misaligned", dict(w=ODD)),
        ("codon_conv2d_fwd", "f16_weights_misaligned", dict(w=ODD, dtype=L.F16)),
        ("codon_conv2d_fwd", "no_kernel_k3_128_128", dict(cin=128, cout=128, x_ctotal=136, y_ctotal=136)),
        ("codon_conv2d_fwd", "no_kernel_k7", dict(ksize=7)),
        ("codon_conv2d_fwd", "no_kernel_k1_64_64", dict(ksize=1)),
        ("codon_conv2d_fwd", "f16_no_kernel_k5_64_128", dict(ksize=5, cout=128, y_ctotal=136, dtype=L.F16)),
        ("codon_conv2d_fwd", "big_image_64_channels", dict(height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_fwd", "order_coff_4_and_big_image", dict(x_ctotal=80, x_coff=4, height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_fwd", "order_big_image_and_no_kernel", dict(ksize=7, height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_fwd", "order_misaligned_and_coff_4", dict(w=ODD, x_ctotal=80, x_coff=4)),
        ("codon_conv2d_fwd", "order_unknown_dtype_and_misaligned", dict(w=ODD, dtype=7)),
        ("codon_conv2d_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv2d_fwd", "k1_batch_65536", dict(batch=65536, ksize=1, cin=128, x_ctotal=136)),
        ("codon_conv2d_sum_into_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv_chain1x1_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv_chain1x1_stats_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv2d_gated_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv2d_gated_emit_fwd", "grid_too_large", dict(batch=1 << 29)),
        ("codon_conv2d_sum_into_fwd", "not_5x5", dict(ksize=3)),
        ("codon_conv2d_sum_into_fwd", "not_64_64", dict(cin=128, x_ctotal=136)),
        ("codon_conv2d_sum_into_fwd", "relu_flag", dict(flags=L.CONV_RELU)),
        ("codon_conv2d_sum_into_fwd", "weights_misaligned", dict(w=ODD)),
        ("codon_conv2d_sum_into_fwd", "sum_overlaps_y", dict(sum=P, r_coff=8)),
        ("codon_conv2d_sum_into_fwd", "order_shape_and_flags", dict(ksize=3, flags=L.CONV_RELU)),
        ("codon_conv2d_sum_into_fwd", "order_flags_and_coff_4", dict(flags=L.CONV_RELU, x_ctotal=80, x_coff=4)),
        ("codon_conv_chain1x1_fwd", "not_5x5", dict(ksize=3)),
        ("codon_conv_chain1x1_fwd", "not_128_128", dict(cin=64, cout=64)),
        ("codon_conv_chain1x1_fwd", "accum_flag", dict(flags=L.CONV_ACCUM_OUT)),
        ("codon_conv_chain1x1_fwd", "f16x3_flag", dict(flags=L.CONV_RELU | L.CONV_F16X3)),
        ("codon_conv_chain1x1_fwd", "w_misaligned", dict(w=ODD)),
        ("codon_conv_chain1x1_fwd", "w_chain_misaligned", dict(w_chain=ODD)),
        ("codon_conv_chain1x1_fwd", "order_shape_and_coff_4", dict(ksize=3, x_ctotal=144, x_coff=4)),
        ("codon_conv_chain1x1_stats_fwd", "choff_32", dict(choff=32)),
        ("codon_conv_chain1x1_stats_fwd", "accum_flag", dict(flags=L.CONV_ACCUM_OUT)),
        ("codon_conv_chain1x1_stats_fwd", "partials_misaligned", dict(partials=P + 4)),
        ("codon_conv_chain1x1_stats_fwd", "not_5x5", dict(ksize=3)),
        ("codon_conv2d_gated_fwd", "x_coff_8", dict(x_coff=8)),
        ("codon_conv2d_gated_fwd", "accum_flag", dict(flags=L.CONV_ACCUM_OUT)),
        ("codon_conv2d_gated_fwd", "weights_misaligned", dict(w=ODD)),
        ("codon_conv2d_gated_fwd", "no_kernel_k5_128_128", dict(ksize=5, cin=128, cout=128, x_ctotal=136, y_ctotal=136,
                                                                inputs=(136, 8))),
        ("codon_conv2d_gated_fwd", "no_kernel_k1_128_64", dict(ksize=1, cin=128, x_ctotal=136, inputs=(136, 8))),
        ("codon_conv2d_gated_fwd", "x_ctotal_76", dict(x_ctotal=76)),
        ("codon_conv2d_gated_fwd", "order_big_image_and_no_kernel", dict(ksize=1, height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_gated_emit_fwd", "x_coff_8", dict(x_coff=8)),
        ("codon_conv2d_gated_emit_fwd", "no_kernel_k1_64_64", dict(ksize=1)),
        ("codon_conv2d_gated_emit_fwd", "x_ctotal_76", dict(x_ctotal=76)),
        ("codon_conv2d_gated_emit_fwd", "order_big_image_and_gated_out_coff_4", dict(height=BIG128[0], width=BIG128[1],
                                                                                      gated_out=(80, 4))),
        ("codon_conv2d_wgrad", "null_dw_immediate", dict(dw=None)),
        ("codon_conv2d_wgrad", "accumulate_3", dict(accumulate=3)),
        ("codon_conv2d_wgrad", "no_kernel_k7", dict(ksize=7)),
        ("codon_conv2d_wgrad", "no_kernel_k3_128_128", dict(cin=128, cout=128, x_ctotal=136, y_ctotal=136)),
        ("codon_conv2d_wgrad", "workspace_too_small", dict(ws_bytes=16)),
        ("codon_conv2d_wgrad", "f16_workspace_too_small", dict(ws_bytes=16, dtype=L.F16)),
        ("codon_conv2d_wgrad", "order_workspace_and_big_image", dict(ws_bytes=16, height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_wgrad", "big_image_with_workspace", dict(ws_bytes=1 << 40, height=BIG128[0], width=BIG128[1])),
        ("codon_conv2d_wgrad", "order_coff_4_and_workspace", dict(ws_bytes=16, x_ctotal=80, x_coff=4)),
        ("codon_conv1x1_bwd", "big_image_with_workspace", dict(ws_bytes=1 << 40, height=BIG128[0], width=BIG128[1])),
        ("codon_conv1x1_bwd", "order_gx_coff_4_and_no_kernel", dict(ksize=3, gx=(144, 4))),
        ("codon_conv1x1_bwd_gated", "big_image_with_workspace", dict(ws_bytes=1 << 40, height=BIG128[0], width=BIG128[1])),
        ("codon_conv1x1_bwd", "null_dw_immediate", dict(dw=None)),
        ("codon_conv1x1_bwd", "accumulate_3", dict(accumulate=3)),
        ("codon_conv1x1_bwd", "weights_misaligned", dict(w=ODD)),
        ("codon_conv1x1_bwd", "not_1x1", dict(ksize=3)),
        ("codon_conv1x1_bwd", "not_128_64", dict(cin=64, x_ctotal=72, gx=(72, 8))),
        ("codon_conv1x1_bwd", "workspace_too_small", dict(ws_bytes=16)),
        ("codon_conv1x1_bwd", "order_misaligned_and_f32", dict(w=ODD, dtype=L.F32)),
        ("codon_conv1x1_bwd_gated", "fcat_base_32", dict(fcat_base=32)),
        ("codon_conv1x1_bwd_gated", "weights_misaligned", dict(w=ODD)),
        ("codon_conv1x1_bwd_gated", "not_1x1", dict(ksize=3)),
        ("codon_conv1x1_bwd_gated", "workspace_too_small", dict(ws_bytes=16)),
        ("codon_conv_form_c8", "no_kernel_k3_128_128", dict(cin=128, cout=128)),
        ("codon_conv_form_c8", "no_kernel_k7", dict(ksize=7)),
        ("codon_conv_form_c8", "f16_no_kernel_k1_64_64", dict(ksize=1, dtype=L.F16)),
        ("codon_conv_pack_weight", "ksize_7", dict(ksize=7)),
        ("codon_conv_pack_weight", "mode_9", dict(mode=9)),
        ("codon_conv_pack_weight", "cin_24", dict(cin=24)),
        ("codon_conv_pack_weight", "cout_48", dict(cout=48)),
        ("codon_conv_pack_weight", "dgrad_cin_48", dict(cin=48, mode=L.PACK_DGRAD)),
        ("codon_conv_pack_weight", "chain_not_64_128", dict(mode=L.PACK_CHAIN1X1)),
        ("codon_conv_pack_weight", "chain_unknown_dtype", dict(mode=L.PACK_CHAIN1X1, ksize=1, cin=128, cout=64, dtype=7)),
        ("codon_conv_pack_weight", "f16x3_bf16", dict(mode=L.PACK_FWD_F16X3)),
        ("codon_stem_pair_fwd", "slices_overlap", dict(yb=P)),
        ("codon_stem_pair_fwd", "order_overlap_and_unknown_dtype", dict(yb=P, dtype=7)),
        ("codon_head_fwd_y16", "y_misaligned", dict(y=ODD)),
        ("codon_head_fwd_y16", "order_f32_and_misaligned", dict(y=ODD, dtype=L.F32)),
        ("codon_cac_stats_fwd", "partials_misaligned", dict(partials=P + 4)),
        ("codon_cac_stats_fwd", "batch_65536", dict(batch=65536)),
        ("codon_cac_stats_fwd", "order_batch_and_coff_4", dict(batch=65536, pre=(80, 4))),
        ("codon_cac_stats_scaled_fwd", "partials_misaligned", dict(partials=P + 4)),
        ("codon_ew_sq_scale", "batch_65536", dict(batch=65536)),
        ("codon_cac_apply_fwd", "batch_65536", dict(batch=65536)),
        ("codon_cac_apply_fwd", "order_coff_4_and_big_image", dict(out_c=(80, 4), height=BIG64[0], width=BIG64[1])),
        ("codon_stencil_1to64", "no_mask_big_image", dict(mask=None, height=BIG64[0], width=BIG64[1])),
        ("codon_conv1ch_wgrad", "null_dw_immediate", dict(dw=None)),
        ("codon_conv1ch_wgrad", "flip_8", dict(flip=8)),
        ("codon_conv1ch_wgrad", "workspace_too_small", dict(ws_bytes=16)),
        ("codon_conv1ch_wgrad", "order_unknown_dtype_and_null", dict(dtype=7, s=None)),
        ("codon_ew_add_mask", "channels_0", dict(channels=0)),
        ("codon_ew_add_mask", "channels_12", dict(channels=12)),
        ("codon_ew_add_mask", "batch_65536", dict(batch=65536)),
        ("codon_ew_add_mask", "big_image_128_channels", dict(channels=128, dst=(136, 8), src=(136, 8), mask=(136, 8),
                                                             height=BIG128[0], width=BIG128[1])),
        ("codon_ew_add_mask", "order_channels_12_and_coff_4", dict(channels=12, dst=(80, 4))),
        ("codon_ew_sum_mask", "nsrc_0", dict(nsrc=0)),
        ("codon_ew_sum_mask", "nsrc_5", dict(nsrc=5)),
        ("codon_ew_sum_mask", "source_aliases_dst", dict(src1=(72, 8, P))),
        ("codon_ew_sum_mask", "channels_12", dict(channels=12)),
        ("codon_ew_sum_mask", "batch_65536", dict(batch=65536)),
        ("codon_ew_sum_mask", "order_big_image_and_src_coff_4", dict(src1=(80, 4, P + 0x200), height=BIG64[0], width=BIG64[1])),
        ("codon_cac_bwd_reduce", "batch_65536", dict(batch=65536)),
        ("codon_cac_bwd_reduce_acc", "batch_65536", dict(batch=65536)),
        ("codon_cac_bwd_reduce_acc", "order_g_in_coff_4_and_big_image", dict(g_in=(80, 4), height=BIG64[0], width=BIG64[1])),
        ("codon_cac_bwd_apply", "batch_65536", dict(batch=65536)),
        ("codon_stem_pair_fwd_guarded", "slices_overlap", dict(yb=P)),
        ("codon_stem_pair_fwd_guarded", "order_overlap_and_unknown_dtype", dict(yb=P, dtype=7)),
        ("codon_head_fwd_y16_guarded", "y_misaligned", dict(y=ODD)),
        ("codon_head_fwd_y16_guarded", "order_f32_and_misaligned", dict(y=ODD, dtype=L.F32)),
        ("codon_lr_codes_to_input", "scale_3", dict(scale=3)),
        ("codon_lr_codes_to_input", "code_bits_12", dict(code_bits=12)),
        ("codon_lr_codes_to_input", "depth_max_0", dict(depth_max=0)),
        ("codon_lr_codes_to_input", "depth_max_8_bit", dict(code_bits=8, depth_max=1000)),
        ("codon_lr_codes_to_input", "lr_height_65537", dict(height=65537)),
        ("codon_lr_codes_to_input", "out_misaligned", dict(out=P + 8)),
        ("codon_lr_codes_to_input", "codes_misaligned", dict(codes=ODD)),
        ("codon_lr_codes_to_input", "order_scale_and_unknown_dtype", dict(scale=3, dtype=7)),
        ("codon_lr_codes_to_input", "order_unknown_dtype_and_code_bits", dict(dtype=7, code_bits=12)),
        ("codon_d4_views", "src1_without_its_outputs", dict(src1=P)),
        ("codon_d4_views", "upright1_without_src1", dict(upright1=P)),
        ("codon_d4_views", "batch_32768", dict(batch=32768)),
        ("codon_d4_views", "order_shape_and_unknown_dtype", dict(height=0, dtype=7)),
        ("codon_d4_views", "order_unknown_dtype_and_batch", dict(dtype=7, batch=32768)),
        ("codon_d4_merge", "batch_32768", dict(batch=32768)),
        ("codon_d4_merge", "order_unknown_dtype_and_batch", dict(dtype=7, batch=32768)),
        ("codon_cast_multi", "n_0", dict(n=0)),
        ("codon_cast_multi", "n_33", dict(n=33)),
        ("codon_cast_multi", "null_src", dict(src=None)),
        ("codon_cast_multi", "count_0", dict(count=0)),
        ("codon_postprocess_u8_dt", "bf16", dict(dtype=L.BF16)),
        ("codon_postprocess_u8_dt", "n_0", dict(n=0)),
        ("codon_postprocess_u16_dt", "depth_max_0", dict(depth_max=0)),
        ("codon_postprocess_u16_dt", "out_misaligned", dict(out=ODD)),
    ]
    ids = [(n, c) for n, c, _ in out + by_hand]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return out + by_hand


def case_id(name, case):
    return f"{name[6:]}.{case}"


def table():
    return {case_id(n, c): list(call(n, o)) for n, c, o in cases()}


if __name__ == "__main__":
    t = table()
    reached = {k: v for k, v in t.items() if v[0] not in (-1, -2)}
    assert not reached, f"not refused before a HIP call: {reached}"
    with open(sys.argv[1], "w") as f:
        json.dump(t, f, indent=1, sort_keys=True)
        f.write("\n")
