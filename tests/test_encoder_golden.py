"""The host builds of the Blosc encoders write the bytes tests/golden/encoder_frames.json records (the commit it names:
the last one before the encoders came to share one frame writer, ``csrc/dsx_blosc_frame.h``).  The other encoder tests
hold the kernels to the host build and the host build to libzstd / liblz4 / c-blosc by decoding, which a change made
to both sides alike passes as long as the frames still decode; this file holds every frame byte and every offset of
``tests/encoder_golden_cases.py`` in place.  Held to the record: ``dsx_blosc_encode_ref_ex`` of the library, the g++
builds of ``tests/host/zstd_enc_check.cpp``, ``zstd_enc_runs_check.cpp`` and ``lz4_enc_check.cpp``, and the stored
frames of the single-frame writers ``dsx_blosc_encode`` and ``dsx_blosc_encode_lz4``.  No GPU needed."""

import os
import subprocess

import numpy as np
import pytest

import encoder_golden_cases as gc
from aind_smartspim_destripe_amd import engine as eng_mod
from aind_smartspim_destripe_amd import mini_zarr

HERE = os.path.dirname(os.path.abspath(__file__))
MODE_ARG = {"literals": 0, "runs": 1}  # <mode> of zstd_enc_runs_check


@pytest.fixture(scope="module")
def golden():
    g = gc.load_golden()
    assert len(g["commit"]) == 40
    return g["digests"]


@pytest.fixture(scope="module")
def cases():
    return gc.cases()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = {}
    for name in ("zstd_enc_check", "zstd_enc_runs_check", "lz4_enc_check"):
        out[name] = str(tmp_path_factory.mktemp("golden") / name)
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", out[name],
                        os.path.join(HERE, "host", name + ".cpp")], check=True)  # fmt: skip
    return out


def _run(exe, tmp_path, chunks, args):
    src, fr, of = (str(tmp_path / x) for x in ("in.raw", "frames.bin", "offsets.bin"))
    chunks.tofile(src)
    nb = chunks.nbytes // len(chunks) if len(chunks) else 0
    count = [] if nb else [str(len(chunks))]  # (chunks of 0 bytes: the file does not say how many)
    subprocess.run([exe, src, str(nb)] + [str(a) for a in args] + [fr, of] + count, check=True)
    with open(fr, "rb") as f:
        return f.read(), np.fromfile(of, np.int64)


def test_the_record_covers_the_cases(golden, cases):
    assert set(golden) == {gc.key(name, mode, clevel) for name, _ in cases for mode, clevel in gc.settings()}


def test_library_host_build_writes_the_recorded_bytes(golden, cases):
    for name, chunks in cases:
        for mode, clevel in gc.settings():
            k = gc.key(name, mode, clevel)
            assert gc.digest(*eng_mod.blosc_encode_ref(chunks, clevel, mode=mode)) == golden[k], k


def test_gxx_builds_write_the_recorded_bytes(golden, cases, exes, tmp_path):
    for name, chunks in cases:
        for mode, clevel in gc.settings():
            k = gc.key(name, mode, clevel)
            if mode == "lz4":
                got = [_run(exes["lz4_enc_check"], tmp_path, chunks, [clevel])]
            else:
                got = [_run(exes["zstd_enc_runs_check"], tmp_path, chunks, [clevel, MODE_ARG[mode]])]
                if mode == "literals":
                    got.append(_run(exes["zstd_enc_check"], tmp_path, chunks, [clevel]))
            for frames, offsets in got:
                assert gc.digest(frames, offsets) == golden[k], k


def test_single_frame_writers_store_the_recorded_frames(golden, cases):
    """``dsx_blosc_encode`` (typesize 2, shuffle) and ``dsx_blosc_encode_lz4`` at clevel 0, and on a buffer under 128
    bytes at the modes' levels: their stored frames, chunk after chunk, are the recorded ones of the batch encoders."""
    by_name = dict(cases)
    picks = [(name, 0) for name in ("2 chunks x 100 bytes", "600 chunks x 256 bytes", "lz4: 40 elements", "lz4: empty",
                                    "3 chunks x (256 KiB + 2 bytes)")]  # fmt: skip
    picks += [("2 chunks x 100 bytes", level) for level in sorted(set(gc.CLEVELS.values()))]  # stored at every level
    for name, clevel in picks:
        chunks = by_name[name]
        assert clevel == 0 or chunks[0].nbytes < 128
        for mode, cname in (("literals", "zstd"), ("lz4", "lz4")):
            if clevel not in (0, gc.CLEVELS[mode]):
                continue
            frames = [mini_zarr.blosc_encode(c.tobytes(), 2, clevel=clevel, shuffle=True, cname=cname) for c in chunks]
            offsets = np.cumsum([0] + [len(f) for f in frames])
            assert all(len(f) == c.nbytes + 16 for f, c in zip(frames, chunks))
            assert gc.digest(b"".join(frames), offsets) == golden[gc.key(name, mode, clevel)], (name, mode, clevel)
