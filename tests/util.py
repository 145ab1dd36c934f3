"""Bit-exact comparison helpers for the parity tests, and a scoped environment for the library's knobs."""
import contextlib
import os

import numpy as np


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def assert_bits_equal(got, want, what=""):
    """Bit-for-bit equality (NaNs compare equal when both are NaN; -0.0 != +0.0)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gb, wb = bits(got), bits(want)
    bad = gb != wb
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError("%s: %d of %d values differ, first at %s: got %s want %s" % (
            what, int(bad.sum()), bad.size, idx.tolist(), got[tuple(idx[0])], want[tuple(idx[0])]))


def miss_equal(got_t, want_t, what=""):
    """Closest-hit distances: negative means miss (any negative value), non-negative must match bit for bit."""
    gm, wm = got_t < 0, want_t < 0
    assert (gm == wm).all(), "%s: hit/miss differs for %d rays" % (what, int((gm != wm).sum()))
    assert_bits_equal(got_t[~wm], want_t[~wm], what)


@contextlib.contextmanager
def env(**values):
    """The given environment variables for the duration of the block (the library reads some knobs when a scene is created and others
    at every render call, so scene creation AND the renders belong inside it); the previous values are restored afterwards."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update({k: str(v) for k, v in values.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
