"""Record every call into libcodon_hip.so as data: the entry's name, every scalar argument and descriptor field, and which
stream it went to -- everything except addresses.  Two host-side versions that bind the same library issue the same
launches exactly when their logs are equal.

    import abi_call_log                      # (tools/ on sys.path, or loaded by file name)
    log = abi_call_log.install()             # after `import codon_amd`, before the calls of interest
    model(x, y)
    abi_call_log.dump(log, "forward.json")

    python tools/abi_call_log.py diff a.json b.json      # exit status 1 and the first difference when they differ

A pointer is recorded as "ptr" / "null"; a stream as s0, s1, ... in order of first use (per_stream() splits a log by it)."""
import ctypes as C
import json
import sys


def _value(v):
    if v is None:
        return "null"
    if isinstance(v, (bool, int, float)):
        return v
    if isinstance(v, bytes):
        return v.decode(errors="replace")
    if hasattr(v, "_obj"):                           # C.byref(structure)
        return _value(v._obj)
    if isinstance(v, C.Structure):
        return {n: _field(getattr(v, n), t) for n, t in v._fields_ if n != "reserved"}
    if isinstance(v, C.Array):
        return [_value(e) for e in v]
    if isinstance(v, C.c_void_p):
        return "ptr" if v.value else "null"
    return type(v).__name__


def _field(v, t):
    if t is C.c_void_p:
        return "ptr" if v else "null"
    if isinstance(v, C.Array):
        if getattr(t, "_type_", None) is C.c_void_p:
            return sum(1 for e in v if e)            # how many are set
        return [_value(e) for e in v]
    return _value(v)


class _Logged:
    """Stands in for the bound library: every codon_* entry is called through and recorded."""

    def __init__(self, lib, signatures, log):
        self._lib, self._sig, self._log, self._streams = lib, signatures, log, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = self._sig.get(name)
        if sig is None:
            return fn
        argtypes = sig[1]
        has_stream = bool(argtypes) and argtypes[-1] is C.c_void_p

        def call(*args):
            rec = []
            for i, (a, t) in enumerate(zip(args, argtypes)):
                if t is C.c_void_p:
                    if has_stream and i == len(argtypes) - 1:
                        h = a.value if isinstance(a, C.c_void_p) else a
                        rec.append("s%d" % self._streams.setdefault(h or 0, len(self._streams)))
                    else:
                        rec.append("ptr" if (a.value if isinstance(a, C.c_void_p) else a) else "null")
                else:
                    rec.append(_value(a))
            r = fn(*args)
            self._log.append([name, rec, r if isinstance(r, int) else _value(r)])
            return r

        self.__dict__[name] = call
        return call


def install():
    """Route codon_amd's library calls through the recorder; returns the list the records are appended to."""
    from codon_amd import _lib as L
    lib = L.load()
    log = []
    L._lib = _Logged(lib._lib if isinstance(lib, _Logged) else lib, L.SIGNATURES, log)
    return log


def per_stream(log):
    out = {}
    for name, args, ret in log:
        s = args[-1] if args and isinstance(args[-1], str) and args[-1][:1] == "s" and args[-1][1:].isdigit() else "-"
        out.setdefault(s, []).append([name, args, ret])
    return out


def dump(log, path):
    with open(path, "w") as f:
        json.dump(log, f)


def diff(a, b):
    """None when the two logs are equal, else a description of the first difference."""
    for i, (ra, rb) in enumerate(zip(a, b)):
        if ra != rb:
            return f"call {i}: {ra} != {rb}"
    if len(a) != len(b):
        return f"{len(a)} calls != {len(b)} calls"
    return None


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "diff":
        sys.exit(__doc__)
    la, lb = (json.load(open(p)) for p in sys.argv[2:])
    d = diff(la, lb)
    print(f"{sys.argv[2]} vs {sys.argv[3]}: " + (d or f"identical ({len(la)} calls, {len(per_stream(la))} streams)"))
    sys.exit(1 if d else 0)
