#!/usr/bin/env python3
"""Bytes of the device Blosc-zstd encoder's two modes against the host writer (zstd level 5), on the host build of the
encoder (no GPU needed): 8 synthetic (64, 128, 128) bricks (the `_bricks(8)` of tests/test_zstd_encoder_host.py), and
the 2 x 2 x 2 means (once and twice) of 8 bricks of twice the size.  Prints one JSON document
(profiles/device_codec_runs_sizes.json)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aind_smartspim_destripe_amd import engine, mini_zarr, synth
from oracle import format_oracle as fo


def bricks(n, shape):
    return np.stack([synth.synthetic_plane(k, shape[0] * 4, shape[1] * shape[2] // 4).reshape(shape) for k in range(n)])


def sizes(chunks):
    chunks = np.ascontiguousarray(chunks, np.uint16)
    lit = len(engine.blosc_encode_ref(chunks, mode="literals")[0])
    runs = len(engine.blosc_encode_ref(chunks, mode="runs")[0])
    host = sum(len(mini_zarr.blosc_encode(c.tobytes(), 2, clevel=3, shuffle=True)) for c in chunks)
    return {"chunks": list(chunks.shape), "raw_bytes": int(chunks.nbytes), "host_writer_bytes": host,
            "entropy_only_bytes": lit, "runs_bytes": runs, "entropy_only_to_host_writer": round(lit / host, 4),
            "runs_to_host_writer": round(runs / host, 4), "runs_to_entropy_only": round(runs / lit, 4)}


big = bricks(8, (128, 256, 256))
levels = [fo.pyramid(b, 3) for b in big]
doc = ({"encoder": "host build (dsx_blosc_encode_ref_ex), clevel 3; host writer: mini_zarr.blosc_encode clevel 3 = zstd level 5",
                  "bricks_8": sizes(bricks(8, (64, 128, 128))),
                  "means_once_of_128x256x256": sizes(np.stack([lv[1] for lv in levels])),
                  "means_twice_of_128x256x256": sizes(np.stack([lv[2] for lv in levels]))})
print("{\n" + ",\n".join(" {}: {}".format(json.dumps(k), json.dumps(v)) for k, v in doc.items()) + "\n}")
