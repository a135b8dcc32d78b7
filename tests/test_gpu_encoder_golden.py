"""The device encoders write the bytes tests/golden/encoder_frames.json records (see tests/test_encoder_golden.py), in
all three modes and at clevel 0, for the ``GPU_CASES`` of tests/encoder_golden_cases.py: an offset scan over three
batches of 256 chunks with coded and memcpyed frames mixed, no chunk at all, chunks stored whole (the workgroups of
every block but the first leave), a full block with the shortest leftover block, a split block with a stored stream
next to a coded one, and an unsplit leftover stream.  A few MB in all; the larger tables stay with the tests that hold
the device to the host build."""

import numpy as np
import pytest

import encoder_golden_cases as gc
from aind_smartspim_destripe_amd import engine as eng_mod

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = eng_mod.DestripeEngine(0)
    yield e
    e.close()


def _device_frames(e, chunks, clevel, mode):
    n = chunks.shape[0]
    nb = chunks.nbytes // n if n else 0
    cap = n * (nb + 16) + 1
    d_src, d_frames, d_off = e.alloc(max(chunks.nbytes, 2)), e.alloc(cap), e.alloc(8 * (n + 1))
    try:
        if chunks.nbytes:
            d_src.upload(chunks)
        e.blosc_encode_device(d_src, n, nb, d_frames, d_off, typesize=2, clevel=clevel, mode=mode)
        e.sync()
        offsets = d_off.download((n + 1,), np.int64)
        assert 0 <= offsets[-1] < cap
        return d_frames.download((cap,), np.uint8)[: offsets[-1]].tobytes(), offsets
    finally:
        for b in (d_src, d_frames, d_off):
            b.free()


@pytest.fixture(scope="module")
def table():
    by_name = dict(gc.cases())
    return gc.load_golden()["digests"], {name: by_name[name] for name in gc.GPU_CASES}


@pytest.mark.parametrize("mode", ["literals", "runs", "lz4"])
def test_device_writes_the_recorded_bytes(engine, table, mode):
    golden, cases = table
    for name, chunks in cases.items():
        for clevel in (gc.CLEVELS[mode], 0):
            got = gc.digest(*_device_frames(engine, chunks, clevel, mode))
            assert got == golden[gc.key(name, mode, clevel)], (name, mode, clevel)
