"""-m gpu tier: the context's caching device pool (nrq_dev_alloc / nrq_dev_free / nrq_dev_trim) on the device.  The pool's logic is
covered on the CPU (tests/test_host_model.py, group b); here the one thing only the device can say: a block that is freed, freed
again (refused) and handed out again never shares its bytes with a block that is still live."""
import ctypes as C

import numpy as np
import pytest

import nanorq_amd

pytestmark = pytest.mark.gpu


def _books(c):
    b = (C.c_size_t * 3)()
    c._L.nrq_dev_pool_books.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    assert c._L.nrq_dev_pool_books(c._h, b) == 0
    return tuple(int(x) for x in b)


def test_a_refused_second_free_and_the_reuse_leave_a_live_block_intact():
    c = nanorq_amd.Context(0)
    n = 200000
    keep = c.alloc(n)                      # stays live throughout
    pattern = (np.arange(n, dtype=np.uint32) * 2654435761 >> 24).astype(np.uint8)
    c.upload(keep, pattern)
    p = c.alloc(n)
    c.memset(p, 0x11, n)
    c.sync()
    c.free(p)
    before = _books(c)
    assert before[:2] == (2, 1)
    with pytest.raises(nanorq_amd.binding.NrqError, match="freed already"):
        c.free(p)                          # used to put the block into the cache a second time
    assert _books(c) == before
    with pytest.raises(nanorq_amd.binding.NrqError, match="not a block"):
        c.free(keep + 4096)
    q1, q2 = c.alloc(n), c.alloc(n)        # the cached block once, then a new one
    assert q1 == p and q2 not in (p, keep) and _books(c)[:2] == (3, 0)
    c.memset(q1, 0xA5, n)
    c.memset(q2, 0x5A, n)
    c.sync()
    assert np.array_equal(c.download(keep, n), pattern)
    assert (c.download(q1, n) == 0xA5).all() and (c.download(q2, n) == 0x5A).all()
    for x in (q1, q2):
        c.free(x)
    c._L.nrq_dev_trim.argtypes = [C.c_void_p]
    assert c._L.nrq_dev_trim(c._h) == 0
    assert _books(c) == (1, 0, 0)
    assert np.array_equal(c.download(keep, n), pattern)
    c.free(keep)
    c.close()
