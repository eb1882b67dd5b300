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


def verdict(say, name, here, parent):
    """here, parent: a variant's medians (two rounds each).  The bar is the parent's own spread: this build's median of its medians
    may not exceed the larger of the parent's."""
    ok = statistics.median(here) <= max(parent)
    say("  %-26s this build %9.1f %9.1f | parent %9.1f %9.1f : %s" % (name, here[0], here[1], parent[0], parent[1], "no slower" if ok else "SLOWER"))
    return ok
