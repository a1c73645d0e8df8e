"""bench.py's command line: a plain run does the timed steps alone, `--full`
adds the rest, and `--dump-outputs DIR` writes what the last timed step
computed (DIR/parity.npy, DIR/revived.npy) so two builds can be compared
output for output.

CPU: `--cpu-workload` (the numpy stand-in for the kernels) through
bench.main() in this process.  GPU: the HIP kernels on a batch larger than
the dump's sample, so the sampled groups are checked against the oracle.
"""
import json
import os

import numpy as np
import pytest

K, L = 10, 1350


def _main(capsys, args):
    import bench
    assert bench.main(args) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _oracle(G):
    import bench
    from oracle import oracle_c as OC
    rows = OC.synth_fixed(bench.SEED_FIXED, 0, G, K, L)
    rc, par = OC.encode_fixed(rows, K, L, G)
    rc2, out = OC.recover_fixed(rows, par, bench.drop_indices(0, G, K), K, L, G)
    assert rc == 0 and rc2 == 0
    return par.reshape(G, L), out.reshape(G, L)


def _check_headline(line, G, steps, warmup):
    assert line["metric"].startswith("FEC XOR encode+recover GiB/s")
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    total = steps * G * 14850 * 2
    # the line rounds value to 0.01 GiB/s and ms_per_step to 0.1 us
    tol = 0.01 * line["value"] + 0.01
    assert abs(line["value"] - total / 2**30 / (line["ms_per_step"] * steps / 1e3)) <= tol


FULL_ONLY = ("one_pass", "recover_inslot", "phase_beside_service", "ceilings", "ragged",
             "ragged_packed", "protect", "entropy", "e2e_fec_gcm", "e2e_pinned_host",
             "connection", "connection_e2e")


def test_dump_groups_is_a_fixed_sample_within_the_size_limit():
    import bench
    small = bench.dump_groups(100)
    assert np.array_equal(small, np.arange(100))
    assert np.array_equal(bench.dump_groups(bench.DUMP_GROUPS), np.arange(bench.DUMP_GROUPS))
    G = 1 << 20
    a, b = bench.dump_groups(G), bench.dump_groups(G)
    assert np.array_equal(a, b)  # the same groups in every run
    assert a.size == bench.DUMP_GROUPS and a[0] == 0 and a[-1] == G - 1
    assert np.all(np.diff(a) > 0)  # ascending, no group twice
    assert len(set(np.diff(a).tolist())) > 100  # not a stride: no residue class is favoured
    # two float32 arrays of the sample at the largest packet the bench accepts
    assert 2 * bench.DUMP_GROUPS * 1452 * 4 <= 64 * 10**6


def test_plain_cpu_workload_dumps_the_last_steps_outputs(capsys, tmp_path):
    G = 96
    d = str(tmp_path / "dump")
    line = _main(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--groups", str(G),
                          "--cpu-workload", "--dump-outputs", d])
    _check_headline(line, G, 3, 1)
    assert line["cpu_baseline"] is None  # a --full leg
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(d)) == ["parity.npy", "revived.npy"]
    par, out = np.load(os.path.join(d, "parity.npy")), np.load(os.path.join(d, "revived.npy"))
    assert par.dtype == np.float32 and out.dtype == np.float32
    assert par.shape == (G, L) and out.shape == (G, L)
    want_par, want_out = _oracle(G)
    assert np.array_equal(par, want_par.astype(np.float32))
    assert np.array_equal(out, want_out.astype(np.float32))
    # the same arguments again: the same files, byte for byte
    d2 = str(tmp_path / "dump2")
    _main(capsys, ["--gpus", "1", "--steps", "3", "--warmup", "1", "--groups", str(G),
                   "--cpu-workload", "--dump-outputs", d2])
    for name in ("parity.npy", "revived.npy"):
        assert open(os.path.join(d, name), "rb").read() == open(os.path.join(d2, name), "rb").read()


@pytest.mark.gpu
def test_plain_gpu_run_is_lean_and_dumps_the_sampled_groups(capsys, tmp_path):
    """5,000 groups: more than the dump's 4,096, so the files hold the seeded
    sample; every sampled group's parity and revived packet equal the oracle's."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    import bench
    G = 5000
    d = str(tmp_path / "dump")
    line = _main(capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--groups", str(G),
                          "--dump-outputs", d])
    _check_headline(line, G, 2, 1)
    assert line["verified"] is None and line["cpu_baseline"] is None  # --full checks and legs
    assert not [k for k in FULL_ONLY if k in line]
    assert line["roofline"]["avg_launch_us"] > 0  # from the timed steps' own events
    idx = bench.dump_groups(G)
    par, out = np.load(os.path.join(d, "parity.npy")), np.load(os.path.join(d, "revived.npy"))
    assert par.dtype == np.float32 and out.dtype == np.float32
    assert par.shape == (bench.DUMP_GROUPS, L) and out.shape == (bench.DUMP_GROUPS, L)
    want_par, want_out = _oracle(G)
    assert np.array_equal(par, want_par[idx].astype(np.float32))
    assert np.array_equal(out, want_out[idx].astype(np.float32))
