"""The eleven C entry points that take a code plane, each as one good call over addresses nothing dereferences, and what a
refusal changes as keyword arguments: tools/make_golden_refusals.py records (status, message) of every violation and of every
pair of two with these, tests/test_code_plane_abi_cpu.py replays the record.  Every call made with them must be refused on the
host, before any HIP call: no address here is memory."""
import ctypes as C
import itertools

from codon_amd import _lib as L
from tests import clean_ref, cloud_ref, fill_ref, guided_fill_ref, jbu_ref, register_ref, stretch_ref


def A(k):
    return 4096 * k                                 # distinct, aligned to anything an entry asks for


RQ = 1311                                           # rint(65536 * 0.02)


def _per_plane(query, h="h", w="w"):
    return lambda lib, a: a["B"] * getattr(lib, query)(a[h], a[w]) if a["B"] > 0 else 0


def _batched(query):
    return lambda lib, a: getattr(lib, query)(a["B"], a["h"], a["w"])


_GUIDED = dict(B=1, h=5, w=7, src=A(1), fmt=L.FILL_U16, top=65535, guide=A(2), row_bytes=28, image_bytes=560, scale=4, tab=A(3))
_LR = dict(B=1, h=5, w=7, scale=4, src=A(1), bits=16, lut=A(2), dm=65535, wt=A(3), out=A(4))
_MAP = dict(B=1, h=5, w=7, src=A(1), bits=16, top=65535, lo_hi=A(2), out=A(3))

# entry -> (the good call's arguments in the ABI's order, less the stream; the workspace the entry needs or None)
ENTRIES = {
    "fill_holes": (dict(B=1, h=5, w=7, src=A(1), fmt=L.FILL_U16, tab=A(2), top=65535, out=A(3), ws=A(4), ws_bytes=None),
                   _per_plane("codon_fill_holes_workspace_bytes")),
    "fill_holes_guided": (dict(_GUIDED, out=A(4), ws=A(5), ws_bytes=None), _per_plane("codon_fill_guided_workspace_bytes")),
    "jbu_upsample": (dict(_GUIDED, stab=A(6), out=A(4), ws=A(5), ws_bytes=None), _per_plane("codon_jbu_workspace_bytes")),
    "register_depth": (dict(B=1, hs=5, ws_=7, src=A(1), fmt=L.FILL_U16, top=65535, rays=A(2), T=(1 << 20, 0, 0), P=(256, 256, 0, 0),
                            ho=3, wo=5, out=A(3), stats=None, ws=A(4), ws_bytes=None),
                       _per_plane("codon_register_workspace_bytes", "ho", "wo")),
    "clean_depth": (dict(B=1, h=5, w=7, src=A(1), fmt=L.FILL_U16, top=65535, tol_abs=2, tol_rel=RQ, support=3, region=16, out=A(2),
                         counts=None, ws=A(3), ws_bytes=None), _batched("codon_clean_workspace_bytes")),
    "cloud_points": (dict(B=1, h=5, w=7, src=A(1), fmt=L.FILL_U16, top=65535, rx=A(2), ry=A(3), span=(-100, 100, -90, 90),
                          m=0.001 / (1 << 20), normals=1, radius=2, tol_abs=2, tol_rel=RQ, color=A(7) + 1, channels=3, body=A(4) + 1,
                          counts=A(5), nmap=None, ws=A(6), ws_bytes=None), _batched("codon_cloud_workspace_bytes")),
    "lr_codes_to_input": (dict(_LR, dtype=L.F32), None),
    "lr_codes_upsample": (dict(_LR), None),
    "code_range": (dict(B=1, h=5, w=7, src=A(1), bits=16, lo_hi=A(2)), None),
    "stretch_codes": (dict(_MAP), None),
    "unstretch_codes": (dict(_MAP), None),
}

_LR_REFUSALS = [{"src": None}, {"lut": None}, {"wt": None}, {"out": None}, {"scale": 5}, {"scale": 0}, {"bits": 12}, {"bits": 8},
                {"bits": 8, "dm": 256}, {"dm": 0}, {"dm": 65536}, {"B": 0}, {"h": 0}, {"w": -1}, {"h": 65537}, {"w": 65537},
                {"h": 40000, "w": 40000}, {"out": A(4) + 8}, {"src": A(1) + 1}]


def _of(refusals, *unaligned):
    """the (kwargs, word) list of a tests/*_ref.py as kwargs alone, then the unaligned-pointer cases"""
    rename = {"trans": "T", "proj": "P"}            # register_ref's two switches are this module's arrays themselves
    return [{rename.get(k, k): v for k, v in kw.items()} for kw, _ in refusals] + [dict([u]) for u in unaligned]


_STRETCH = _of(stretch_ref.REFUSALS, ("out", A(3) + 1))
VIOLATIONS = {
    "fill_holes": _of(fill_ref.REFUSALS, ("src", A(1) + 1), ("out", A(3) + 1), ("ws", A(4) + 1)) + [{"fmt": 2, "top": 255, "out": A(3) + 2}],
    "fill_holes_guided": _of(guided_fill_ref.REFUSALS, ("src", A(1) + 1), ("out", A(4) + 1), ("tab", A(3) + 1), ("ws", A(5) + 8)),
    "jbu_upsample": _of(jbu_ref.REFUSALS, ("src", A(1) + 1), ("out", A(4) + 8), ("tab", A(3) + 1), ("stab", A(6) + 1), ("ws", A(5) + 8)),
    "register_depth": _of(register_ref.REFUSALS, ("src", A(1) + 1), ("out", A(3) + 1), ("rays", A(2) + 2), ("stats", A(5) + 2),
                          ("ws", A(4) + 8)),
    "clean_depth": _of(clean_ref.REFUSALS, ("src", A(1) + 1), ("out", A(2) + 1), ("counts", A(5) + 2), ("ws", A(3) + 8)),
    "cloud_points": _of(cloud_ref.REFUSALS, ("src", A(1) + 1), ("rx", A(2) + 2), ("ry", A(3) + 1), ("counts", A(5) + 2), ("ws", A(6) + 8)),
    "lr_codes_to_input": _LR_REFUSALS + [{"dtype": 3}, {"dtype": -1}],
    "lr_codes_upsample": _LR_REFUSALS + [{"out": "src"}],
    "code_range": [kw for kw in _of(stretch_ref.REFUSALS) if "top" not in kw and "out" not in kw],
    "stretch_codes": _STRETCH,
    "unstretch_codes": _STRETCH,
}


def cases(violations):
    """every violation alone, then every pair of two, the second's arguments over the first's"""
    return list(violations) + [{**a, **b} for a, b in itertools.combinations(violations, 2)]


def call(lib, entry, kw):
    """(status, message) of `entry`'s good call with the arguments of `kw` changed.  A pointer is None, an address, the name of
    another argument (its address: an alias), "odd" (its own address plus one) or "set" (the body's: cloud's normal map);
    ws_bytes is None for what the entry needs, "short" for one byte less"""
    good, need = ENTRIES[entry]
    unknown = set(kw) - set(good)
    assert not unknown, (entry, unknown)
    a = {**good, **kw}
    args = []
    for (name, v), ctype in zip(a.items(), L.SIGNATURES["codon_" + entry][1]):
        if name == "ws_bytes":
            n = need(lib, a)
            v = n if v is None else max(n - 1, 0)
        elif ctype is C.c_void_p:
            if isinstance(v, str):
                v = good[name] + 1 if v == "odd" else a["body" if v == "set" else v]
            v = None if v is None else C.c_void_p(v)
        elif v is not None and isinstance(v, (tuple, list)):
            v = (ctype._type_ * len(v))(*v)
        args.append(v)
    st = getattr(lib, "codon_" + entry)(*args, None)
    return st, lib.codon_last_error_string().decode()
