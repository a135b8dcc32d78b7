"""The inputs whose encoded bytes tests/golden/encoder_frames.json pins (tools/make_golden_encoder_frames.py recorded
them at the commit named in the file), shared by tests/test_encoder_golden.py (the host builds) and
tests/test_gpu_encoder_golden.py (the kernels).

Every case is ``(name, chunks)``: ``chunks`` a uint16 array ``[n, elements]`` -- n chunks of one size, one call of an
encoder.  Every case is encoded in every mode of ``engine.ZENC_MODES`` at the mode's level of ``CLEVELS`` and at level 0
(stored frames); the record holds, per ``key(name, mode, clevel)``, the sha256 of the packed frames and of the int64
offsets.  The tables of the other encoder tests are taken whole, so a frame byte that changes shows here even where
the change was made to the host build and the kernels alike and still decodes."""

import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_frames.json")
CLEVELS = {"literals": 3, "runs": 3, "lz4": 5}
BLOCK = 256 * 1024
# the cases the kernels are held to (the larger tables stay with the device-against-host tests)
GPU_CASES = ("600 chunks x 256 bytes", "0 chunks", "2 chunks x 100 bytes", "3 chunks x (256 KiB + 2 bytes)",
             "lz4: one full block of noise and zeros", "lz4: full block + 12-byte leftover stream")  # fmt: skip


def _device_codec_inputs():
    """The six inputs of tests/test_gpu_device_codec.py::test_device_frames_are_the_host_builds_bytes."""
    from aind_smartspim_destripe_amd import synth

    rs = np.random.RandomState(11)
    bricks = np.stack([synth.synthetic_plane(k, 256, 4096).reshape(64, 128, 128) for k in range(6)])
    out = [bricks, np.zeros((3, 64, 64, 64), np.uint16), rs.randint(0, 65536, (3, 100000)).astype(np.uint16),
           rs.randint(0, 3, (5, 40)).astype(np.uint16),
           (rs.poisson(40, (4, 3 * 65536 + 1000)) + 0x300).astype(np.uint16)]  # fmt: skip
    fib = np.repeat(np.arange(24), [int(round(1.618**k)) for k in range(24)])[:131072]
    out.append(np.stack([np.resize(rs.permutation(fib), 131072), np.arange(131072) % 129]).astype(np.uint16) | 0x700)
    return out


def _mixed_small_chunks(rs, n=600, elements=128):
    """Chunk i is zeros, noise or a 3-symbol alphabet by i % 3: coded and memcpyed frames mixed, and an offset scan
    over three batches of 256 chunks."""
    a = np.zeros((n, elements), np.uint16)
    a[1::3] = rs.randint(0, 65536, a[1::3].shape)
    a[2::3] = rs.randint(0, 3, a[2::3].shape)
    return a


def cases():
    import lz4_enc_cases as lc
    import test_zstd_encoder_runs_host as runs

    out = [("lz4: " + name, c) for name, c in lc.cases()]
    out.append(("lz4: image bricks", lc.image_bricks()))
    out += [("runs: " + name, c) for name, c in runs.edge_cases()]
    out += [("device codec input {}".format(i), c) for i, c in enumerate(_device_codec_inputs())]
    rs = np.random.RandomState(600)
    out.append(("600 chunks x 256 bytes", _mixed_small_chunks(rs)))
    out.append(("0 chunks", np.zeros((0, 64), np.uint16)))
    out.append(("2 chunks x 100 bytes", rs.randint(0, 3, (2, 50))))  # stored whole at every level
    ne = BLOCK // 2 + 1  # a full block and the shortest leftover block
    out.append(("3 chunks x (256 KiB + 2 bytes)",
                np.stack([rs.randint(0, 3, ne), rs.poisson(40, ne) + 0x300, rs.randint(0, 256, ne)])))  # fmt: skip
    out = [(name, np.ascontiguousarray(c, np.uint16).reshape(len(c), int(np.prod(c.shape[1:])))) for name, c in out]
    assert len({name for name, _ in out}) == len(out)
    return out


def settings():
    """``(mode, clevel)`` of every recorded encoding of a case."""
    return [(mode, clevel) for mode in ("literals", "runs", "lz4") for clevel in (CLEVELS[mode], 0)]


def key(name, mode, clevel):
    return "{} | {} | clevel {}".format(name, mode, clevel)


def digest(frames, offsets):
    offsets = np.ascontiguousarray(offsets, "<i8")
    return {"frames": hashlib.sha256(bytes(frames)).hexdigest(), "offsets": hashlib.sha256(offsets.tobytes()).hexdigest(),
            "bytes": int(offsets[-1])}  # fmt: skip


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
