"""Inputs of the stack-rank tests (``tests/test_stack_rank_host.py``, ``tests/test_gpu_stack_rank.py``): built once,
never modified.  A case is ``(name, stack[n, P], lo, hi, q_milli, lead)``: ``stack`` is a uint16 view ``lead`` elements
into its own flat buffer (``lead`` is 0, or 1 for the stack that starts 2 bytes past an aligned address), and
``expected(case)`` is the contract restated with ``np.sort`` on the masked columns and the INTEGER rank rule
``k = (q * (m - 1)) // 1000`` -- not ``np.percentile``, whose float rule gives another rank for 41 ``(m, q)`` pairs."""

import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name stack lo hi q_milli lead")
FULL = (0, 65535)
ALL_Q = (0, 500, 500, 1000)  # several quantiles in one call, one of them twice
N_EDGES = (1, 2, 3, 127, 128, 129, 255, 256, 257, 512)  # both sides of each tile-width switch, and the limits
P_EDGES = (1, 35, 64, 65, 256, 257)  # 35 = 5 x 7: odd, so planes start misaligned, and smaller than any tile
P_RAGGED = 1961  # 37 x 53: several blocks and a ragged last tile
P_VEC = 2048  # a multiple of 8: the 16-byte body when the base is aligned


def _frozen(a):
    a.setflags(write=False)
    return a


def _noise(seed, n, P, low=0, high=65536):
    return _frozen(np.random.RandomState(seed).randint(low, high, (n, P)).astype(np.uint16))


def _ranks(seed, n, P):
    """Per pixel a permutation of ``arange(n) * 128``: the k-th smallest is ``128 k``, and with n = 512 the values cross
    0x8000."""
    rs = np.random.RandomState(seed)
    order = np.argsort(rs.rand(n, P), axis=0)
    return _frozen((order * 128).astype(np.uint16))


def _guarded(seed, n, P):
    """The noise stack one element into a buffer whose first and last element are guards."""
    buf = np.full(n * P + 2, 0xFFFF, np.uint16)
    buf[1:-1] = np.random.RandomState(seed).randint(0, 65535, n * P)
    return _frozen(buf)[1:-1].reshape(n, P)


def _sparse_window(seed, n, P):
    """Values below the window (lo = 1000) everywhere, but every second pixel has exactly one plane inside it: pixels
    with m = 0 and pixels with m = 1."""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 1000, (n, P)).astype(np.uint16)
    for p in range(0, P, 2):
        a[rs.randint(n), p] = 1000 + rs.randint(0, 64000)
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, stack, window=FULL, q=ALL_Q, lead=0):
        out.append(Case(name, stack, window[0], window[1], tuple(q), lead))

    for i, n in enumerate(N_EDGES):  # every n edge on several blocks with a ragged last tile
        add("noise_n{}_p{}".format(n, P_RAGGED), _noise(100 + i, n, P_RAGGED))
    for i, P in enumerate(P_EDGES):  # every P edge, one thread per pixel and four
        add("ranks_n512_p{}".format(P), _ranks(200 + i, 512, P))
        add("noise_n3_p{}".format(P), _noise(220 + i, 3, P), q=(500,))
    add("noise_n129_p35", _noise(240, 129, 35), q=(500,))
    for q in (0, 500, 1000):  # each alone
        add("noise_n129_p257_q{}".format(q), _noise(241, 129, 257), q=(q,))
    for n in (128, 256, 512):  # 16-byte body at every tile width
        add("vec_n{}_p{}".format(n, P_VEC), _noise(250 + n, n, P_VEC), q=(500, 50))
    add("guarded_n128_p{}".format(P_VEC), _guarded(260, 128, P_VEC), q=(500, 50), lead=1)  # the 2-byte body
    for v in (0, 150, 65535):
        add("constant_{}".format(v), _frozen(np.full((3, 65), v, np.uint16)), q=(0, 500, 1000))
    add("two_valued_n2", _noise(270, 2, 65, 100, 102))  # lower median of two
    add("two_valued_n256", _noise(271, 256, 65, 100, 102))
    add("float_rule_m101_q290", _noise(272, 101, 35), q=(290,))  # floor(0.29 * 100) is 28, 290 * 100 // 1000 is 29
    add("window_lo_eq_hi", _noise(273, 129, 257, 149, 152), window=(150, 150))
    add("window_sparse_n3", _sparse_window(274, 3, 65), window=(1000, 65535))
    add("window_sparse_n257", _sparse_window(275, 257, 65), window=(1000, 65535))
    add("window_inner_n257", _noise(276, 257, 257), window=(20000, 50000))  # values at and above 0x8000 on both sides
    return tuple(out)


def ids():
    return [c.name for c in cases()]


def rank_of(q_milli, m):
    return (q_milli * (m - 1)) // 1000


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = {c.name: c for c in cases()}[name]
    n, P = c.stack.shape
    out = np.zeros((len(c.q_milli), P), np.uint16)
    valid = np.zeros(P, np.uint16)
    for p in range(P):
        col = c.stack[:, p]
        v = np.sort(col[(col >= c.lo) & (col <= c.hi)])
        valid[p] = v.size
        if v.size:
            for i, q in enumerate(c.q_milli):
                out[i, p] = v[rank_of(q, v.size)]
    return _frozen(out), _frozen(valid)


def expected(case):
    """``(out uint16 [n_q, P], valid uint16 [P])`` of a case."""
    return _expected(case.name)
