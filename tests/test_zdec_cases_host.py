"""The tables of tests/zdec_cases.py through the host build of the device decoder (``dsx_blosc_decode_ref``): the zstd
mode corpus against the bytes libzstd was given (plain, byte- and bit-shuffled), the proof that the frames ask for every
path of the device driver, the layout sweep between canary bytes, and the malformed zstd tasks -- each of which also
runs under ASan / UBSan here before tests/test_gpu_zdec_cases.py hands it to the kernel.  No GPU needed."""

import os
import struct
import subprocess

import numpy as np
import pytest

import blosc_any_frames as baf
import test_zstd_decoder_host as zh
import zdec_cases as zc
from aind_smartspim_destripe_amd import engine as eng_mod


@pytest.fixture(scope="module")
def frames():
    return zc.mode_frames()


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return zc.build_check_exe(str(tmp_path_factory.mktemp("zc") / "zstd_dec_check"))


@pytest.fixture(scope="module")
def asan_zstd(tmp_path_factory):
    return zc.build_check_exe(str(tmp_path_factory.mktemp("zc_asan") / "zstd_dec_check"), sanitize=True)


@pytest.fixture(scope="module")
def asan_tasks(tmp_path_factory):
    return zc.build_task_exe(tmp_path_factory, sanitize=True)


# ---- the helpers themselves --------------------------------------------------------------------------------------------
def test_numpy_inverses_of_the_shuffles():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 15, 16, 17, 18, 30, 32, 33, 160, 161, 1552, 4096, 70000, 70001):
        raw = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert zc.unshuffle2(baf.shuffle2(raw)) == raw, n
        assert zc.unbitshuffle2(baf.bitshuffle2(raw)) == raw, n
        if (n // 2) % 8:
            assert baf.bitshuffle2(raw) == raw and zc.unbitshuffle2(raw) == raw, n  # left as it is
    # not only inverse to each other: written out for one buffer
    assert zc.unshuffle2(bytes([1, 2, 3, 11, 12, 13, 9])) == bytes([1, 11, 2, 12, 3, 13, 9])
    raw = bytes(range(16))  # 8 elements: row 8 s + b holds bit b of byte s of all 8
    sh = baf.bitshuffle2(raw)
    for s in range(2):
        for b in range(8):
            want = sum(((raw[2 * k + s] >> b) & 1) << k for k in range(8))
            assert sh[8 * s + b] == want
    assert zc.unbitshuffle2(sh) == raw


def test_kernel_constants_are_read_from_the_header():
    k = zc.kernel_constants()
    assert set(k) == {"kSeqBatch", "kLitWin", "kLz4Win"} and all(v >= 64 for v in k.values())


def test_pattern_has_no_short_period():
    p = zc.pattern(4096)
    assert p[0] == 7 and p[1] == 138 and len(set(p[:256].tolist())) == 256


# ---- A -------------------------------------------------------------------------------------------------------------------
def test_periodic_frames_are_one_overlapping_match(frames, check_exe, tmp_path):
    """libzstd writes each periodic buffer as a match of offset p that overlaps its own output."""
    per = [f for f in frames if f[0].startswith("period")]
    assert len(per) == 2 * len(zc.PERIODS)
    for (name, _, data), s in zip(per, zc.frame_stats(check_exe, tmp_path, per)):
        p = int(name[len("period") : name.index("@")])
        assert data[p:] == data[:-p] and len(set(data[:p])) == p
        assert s["status"] == 0 and (s["pat_div"] if 64 % p == 0 else s["pat_nodiv"]) >= 1, (name, s)


def test_mode_frames_decode_to_what_libzstd_was_given(frames, check_exe, tmp_path):
    """Plain, byte-shuffled and bit-shuffled: one table each, every status 0, every byte, no byte outside."""
    for flag in zc.FLAGS:
        t = zc.mode_table(frames, flag)
        out, st = zc.run_ref(t)
        zc.check(t, out, st, "host build, flag {:#x}".format(flag))
    print("section A: {} tasks per table, 3 tables".format(len(frames)))
    added = [f for f in frames if f[0].startswith(("period", "chained", "skewed"))]
    res = zh._decode_gxx(check_exe, tmp_path, [(f, len(d)) for _, f, d in added])  # the g++ build on the added corpus
    for (name, _, data), (st, got) in zip(added, res):
        assert st == 0 and got == data, name


def test_mode_frames_cover_every_path_of_the_device_driver(frames, check_exe, tmp_path):
    cov = zc.coverage(frames, zc.frame_stats(check_exe, tmp_path, frames))
    print(zc.coverage_report(cov))
    assert not zc.missing_cases(cov), zc.missing_cases(cov)


def test_stats_walker_on_the_hand_frame(check_exe, tmp_path):
    """One sequence: 2 literals, then offset 1, 10 bytes -- known by construction."""
    s = zc.frame_stats(check_exe, tmp_path, [("hand",) + zh._hand_frame()])[0]
    assert s["status"] == 0 and s["seqs"] == 1 and s["off1"] == 1 and s["pat_div"] == 1 and s["pat_nodiv"] == 0
    assert s["bar_own_lit"] == 1 and s["barriers"] == 1 and s["off_ge_ml"] == 0 and s["comp_blocks"] == 1
    assert s["max_seq"] == 1 and s["huf1"] == s["huf4"] == 0 and s["repeat"] == 0


def test_blosc_level_frames_through_reader_and_ref(tmp_path):
    cases = zc.blosc_level_frames()
    assert len(cases) == 3 * len(zh.LEVELS)
    paths = []
    for i, (name, frame, raw) in enumerate(cases):
        paths.append(str(tmp_path / "c{:02d}".format(i)))
        with open(paths[-1], "wb") as f:
            f.write(frame)
    cb = len(cases[0][2])
    packed, tasks, routes = eng_mod.io_read_frames(paths, cb)
    assert all(int(r) == eng_mod.ROUTE_DEVICE for r in routes)
    out, st = eng_mod.blosc_decode_ref(packed, tasks, cb * len(cases))
    assert not st.any()
    for i, (name, _, raw) in enumerate(cases):
        assert out[i * cb : (i + 1) * cb].tobytes() == raw, name


# ---- B -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layout():
    return zc.layout_table()


def test_layout_sweep(layout):
    t, facts = layout
    assert len(t.rows) >= 393
    ends = sorted((r[1], r[1] + r[3]) for r in t.rows)
    assert all(b[0] - a[1] >= zc.GAP for a, b in zip(ends, ends[1:]))  # the canary between neighbouring outputs
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "host build")
    print("section B: {} tasks".format(len(t.rows)))


def test_layout_sweep_takes_every_path(layout):
    paths = zc.layout_paths(layout[1])
    print("\n".join("{:<60} {}".format(k, v) for k, v in sorted(paths.items())))
    assert len(paths) >= 12 + 4 + 16 + 4
    assert not [k for k, v in paths.items() if v == 0], [k for k, v in paths.items() if v == 0]


def test_lz4_window_walk_follows_the_python_decoder():
    stream, raw = zc.lz4_window_stream()
    assert baf.lz4_decompress_py(stream, len(raw)) == raw
    w = zc.lz4_window_walk(stream)
    assert len(stream) > zc.kernel_constants()["kLz4Win"] and w["refills"] >= 2 and w["staged"] and w["crossing"]
    # a stream that fits the window is read with one fill and every literal run lies in it
    small = baf.Lz4Asm().lit(b"abcdefgh").match(3, 20).lit(b"12345").end()[0]
    assert zc.lz4_window_walk(small) == {"staged": 2, "crossing": 0, "outside": 0, "refills": 1}


# ---- C -------------------------------------------------------------------------------------------------------------------
def test_malformed_tasks_under_sanitizers_first(asan_zstd, asan_tasks, tmp_path):
    """Every input of section C through the ASan / UBSan builds: as a task (``zdec_task_check``), and the bare frames
    through ``zstd_dec_check`` too."""
    cases = zc.malformed_cases()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    rec, out = str(tmp_path / "tasks.bin"), str(tmp_path / "tasks.out")
    zc.write_records(rec, [(b, n, kind) for _, b, n, kind, _ in cases])
    r = subprocess.run([asan_tasks, "decode", rec, out], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    blob = open(out, "rb").read()
    assert len(blob) == 4 * len(cases)  # a status each and no output: none of them decodes
    got = struct.unpack("<{}i".format(len(cases)), blob)
    for (name, _, _, _, want), st in zip(cases, got):
        assert st != 0 and (want is None or st == want), (name, st, want)
    bare = [(b, n) for _, b, n, kind, _ in cases if kind == eng_mod.TASK_ZSTD]
    rec = str(tmp_path / "frames.bin")
    zc.write_records(rec, bare)
    r = subprocess.run([asan_zstd, "decode", rec, out], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert len(open(out, "rb").read()) == 4 * len(bare)


def test_malformed_tasks_between_good_ones(frames):
    t = zc.malformed_table(zc.good_neighbours(frames))
    cases = zc.malformed_cases()
    cuts = sum(len(f[0]) + 1 for f in (zh._hand_frame(), zh._hand_frame_fcs8()))  # every truncation + one appended
    assert len(t.rows) == 2 * len(cases) + 1 and len(cases) == 9 + cuts + 1 + 3
    documented = {k: v[2] for k, v in zh._broken_frames().items()}
    assert all(st == documented[name] for name, _, _, _, st in cases if name in documented) and len(documented) == 9
    out, st = zc.run_ref(t)
    zc.check(t, out, st, "host build")
    assert all(int(s) != 0 for s, e in zip(st, t.expect) if e is None)
    print("section C: {} tasks ({} malformed)".format(len(t.rows), len(cases)))
