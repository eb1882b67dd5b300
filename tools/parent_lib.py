"""--parent-lib of the kbench tools: the parent commit's library (tools/build_variant.sh in a checkout of the parent) loaded beside
this build's, and the package's wrappers called through either -- a second CDLL on the same argument structs."""
import contextlib
import ctypes
import os
import statistics

from dynamicfusion_body_amd import _lib


class _Mixed:
    """The loaded library with the entry points `names` taken from `parent`."""

    def __init__(self, here, parent, names):
        self._here = here
        for n in names:
            fn = getattr(parent, n)
            fn.restype, fn.argtypes = _lib._SIGNATURES[n]
            setattr(self, n, fn)

    def __getattr__(self, name):
        return getattr(self._here, name)


def open_parent(path, names):
    return _Mixed(_lib.load(), ctypes.CDLL(os.path.abspath(path)), names)


@contextlib.contextmanager
def through(lib):
    """kernels.* inside this block call `lib` (None: this build's library)."""
    keep = _lib.load()
    _lib._lib = keep if lib is None else lib
    try:
        yield
    finally:
        _lib._lib = keep


def pair_order(variants, rnd):
    """variants: (this build, parent) pairs in a flat list.  The second of a pair runs on the data its twin has just pulled into the
    cache, so the pairs swap places from round to round: each library is timed once in either position."""
    return variants if rnd == 0 else [variants[i ^ 1] for i in range(len(variants))]


def against_parent(say, what, call, names, path, reps=20):
    """One workload through this build's library and through the parent's entry points `names`.  call(lib) runs it (kernels.* and
    the other wrappers inside it go through `lib` too) and returns its outputs, a sequence of tensors (None entries are skipped).
    The outputs are compared bit for bit; then both libraries are timed by HIP events around call(), alternating (pair_order), two
    rounds of `reps` each after two warm repetitions, and judged by verdict().  Returns (identical, no slower)."""
    import torch
    here, parent = _lib.load(), open_parent(path, names)

    def run(lib):
        with through(lib):
            return call(lib)

    def raw(t):
        return t.contiguous().reshape(-1).view(torch.uint8)
    outs = []
    for lib in (here, parent):
        outs.append([t.clone() for t in run(lib) if t is not None])
        torch.cuda.synchronize()
    same = len(outs[0]) == len(outs[1]) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(raw(x), raw(y)) for x, y in zip(*outs))
    say("%s: %d outputs through this build's library and the parent's: %s" % (what, len(outs[0]), "identical" if same else "DIFFER"))
    variants = [("this build", here), ("parent", parent)]
    times = {(name, rnd): [] for name, _ in variants for rnd in (0, 1)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps + 2):
        for rnd in (0, 1):
            for name, lib in pair_order(variants, rnd):
                e0.record()
                run(lib)
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[(name, rnd)].append(e0.elapsed_time(e1) * 1e3)
    med = {name: [statistics.median(times[(name, rnd)]) for rnd in (0, 1)] for name, _ in variants}
    return same, verdict(say, what + " (us)", med["this build"], med["parent"])


def verdict(say, name, here, parent):
    """here, parent: a variant's medians (two rounds each).  The bar is the parent's own spread: this build's median of its medians
    may not exceed the larger of the parent's."""
    ok = statistics.median(here) <= max(parent)
    say("  %-26s this build %9.1f %9.1f | parent %9.1f %9.1f : %s" % (name, here[0], here[1], parent[0], parent[1], "no slower" if ok else "SLOWER"))
    return ok
