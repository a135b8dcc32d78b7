"""One rank of a multi-rank ``destripe_channel`` run for tests/test_gpu_fused_pyramid.py (one process per rank; RANK /
WORLD_SIZE / DSX_RDZV_DIR in the environment, all ranks on GPU 0 of the one-GPU box).  ``argv[3]`` = ``fused`` turns
``fused_pyramid`` on.  Prints one JSON line."""

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from aind_smartspim_destripe_amd import distributed, engine, synth  # noqa: E402
from aind_smartspim_destripe_amd import zarr_destriper as zd  # noqa: E402


def main():
    root, results, fused = sys.argv[1], sys.argv[2], sys.argv[3] == "fused"
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    multiscale_calls = []
    real = zd.compute_multiscale

    def counting(*a, **k):
        multiscale_calls.append(1)
        return real(*a, **k)

    zd.compute_multiscale = counting
    eng = engine.DestripeEngine(0)
    group = distributed.RankGroup.from_env(eng)
    d = os.path.join(root, "derivatives")
    done = zd.destripe_channel(
        zarr_dataset_path=os.path.join(root, "data"), channel_name="Ex_488_Em_525", results_folder=results,
        derivatives_path=d, xyz_resolution=[1.8, 1.8, 2.0],
        estimated_channel_flats=[os.path.join(d, "flat_0.tif"), os.path.join(d, "flat_1.tif")],
        laser_tiles={"0": ["431040_368180"], "1": ["431040_394100"]},
        parameters={"cells_config": synth.CELLS_CONFIG, "no_cells_config": synth.NO_CELLS_CONFIG},
        prediction_chunksize=(4, 64, 96), output_chunks=(1, 1, 4, 32, 32), compressor="zlib", n_levels=3,
        rank=rank, world_size=world, device=0, group=group if world > 1 or group.active else None,
        fused_pyramid=fused)  # fmt: skip
    out = {"rank": rank, "done": done, "z_range": list(zd.LAST_RUN["z_range"]),
           "fused_pyramid": zd.LAST_RUN["fused_pyramid"], "pyramid_levels": zd.LAST_RUN["pyramid_levels"],
           "multiscale_calls": len(multiscale_calls)}  # fmt: skip
    group.close()
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
