"""bench.py --dump-outputs: the files hold what the last timed step of the bench's own step loop
(bench.Runner / bench.measure, device-record path) handed its caller -- the per-frame results equal
op_fetch_results of that step, the maps equal op_fetch_maps -- in float32 / float64, within the size
budgets (sampled by a fixed seed past them), and identical from run to run."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, load_golden, pkg_module

B = 3


def test_bench_has_the_full_and_dump_options():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs DIR" in p.stdout


def _run_and_dump(bench, lib, ctx, gather, path, steps):
    Fr = pkg_module("frames")
    args = argparse.Namespace(precise=False, graph=0)
    run = bench.Runner(lib, Fr, ctx, args, B, 368, 368, 0, 1, gather)
    try:
        bench.measure(run, ctx, None, steps, 1, False)
        bench.dump_outputs(str(path), run, ctx, B)
        want = ctx.fetch_results(0, B)  # the last timed step, read synchronously
        maps = np.concatenate(ctx.fetch_maps(0, B), axis=1)
    finally:
        run.close()
    return {n[:-4]: np.load(os.path.join(str(path), n)) for n in os.listdir(str(path))}, want, maps, run


@pytest.mark.gpu
def test_dump_holds_the_last_timed_step(ctx, lib, tmp_path, monkeypatch):
    import bench
    d = load_golden("six_people")
    ctx.stage_frames(np.zeros((B, 368, 368, 3), np.uint8))
    ctx.stage_maps(np.concatenate([d["paf_low"], d["heat_low"]])[None].repeat(B, axis=0))
    ctx.use_staged_maps(True)
    Fr = pkg_module("frames")
    gather = bench.make_gather(Fr, ctx, Fr.SocketTransport(0, 1), 1)
    try:
        assert gather.device, gather.label
        got, want, maps, run = _run_and_dump(bench, lib, ctx, gather, tmp_path / "a", 3)
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(a.nbytes for a in got.values()) <= 64 << 20
        # the third timed step after one warm-up is step 3 of the run: frame ids 9..11
        assert got["frame_ids"].tolist() == [9.0, 10.0, 11.0] and not got["status"].any()
        assert run.persons == 3 * sum(r.n_persons for _, _, r in want) > 0
        for i, (p, s, r) in enumerate(want):
            k = r.n_persons
            assert got["n_persons"][i] == k and got["n_peaks"][i] == r.n_peaks
            assert np.array_equal(got["poses"][i, :k], p) and np.array_equal(got["scores"][i, :k], s)
            assert not got["poses"][i, k:].any() and not got["scores"][i, k:].any()
        assert got["maps_frames"].tolist() == [0.0, 1.0, 2.0] and np.array_equal(got["maps"], maps)
        assert np.abs(maps).max() > 0

        # past the budgets: a seeded sample of the frames, then of one frame's positions -- new runs
        # with the same arguments, held to the first run's arrays
        frame_bytes = maps[0].nbytes
        monkeypatch.setattr(bench, "DUMP_MAP_BYTES", 2 * frame_bytes)
        monkeypatch.setattr(bench, "DUMP_POSE_BYTES", 2 * got["poses"][0].nbytes + 2 * got["scores"][0].nbytes)
        some = _run_and_dump(bench, lib, ctx, gather, tmp_path / "c", 3)[0]
        f = some["maps_frames"].astype(int)
        assert len(f) == 2 and np.array_equal(some["maps"], maps[f])
        ids = (some["frame_ids"] - 9).astype(int)
        assert len(ids) == 2 and np.array_equal(some["poses"], got["poses"][ids])
        monkeypatch.setattr(bench, "DUMP_MAP_BYTES", frame_bytes // 4)
        few = _run_and_dump(bench, lib, ctx, gather, tmp_path / "d", 3)[0]
        idx = few["maps_index"].astype(np.int64)
        assert few["maps"].shape == (1, frame_bytes // 64) and np.array_equal(few["maps"][0], maps[0].reshape(-1)[idx])
    finally:
        if gather.device:
            gather.g.close()
        ctx.profile_classes(list(ctx.PROFILE_CLASSES))
        ctx.use_staged_maps(False)
