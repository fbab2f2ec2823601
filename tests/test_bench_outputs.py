"""`bench.py --dump-outputs DIR`: after the timed steps the arrays the timed path computed in its last step are written as DIR/<name>.npy
(float64, at most 64 MB), so that two builds can be compared output for output; `--steps` sets the number of timed steps.  The GPU tests tie
the dumped ciphertext words to the digest the JSON line reports for the same run, and the decrypted logits to the run's own verification."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BENCH_FORCE_DIST", "BENCH_SELF_LAUNCH"):
        env.pop(k, None)
    return env


def _run(*args, timeout=1200):
    r = subprocess.run([sys.executable, BENCH, *args], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert out and all(f.endswith(".npy") for f in os.listdir(d))
    assert all(a.dtype == np.float64 for a in out.values())
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    return out


def test_dump_writes_exact_float64_and_keeps_to_the_limit(tmp_path):
    import bench
    words = np.array([[0, 1, (1 << 49) - 1], [12345, (1 << 53) - 1, 7]], dtype=np.uint64)
    bench.dump_outputs(str(tmp_path / "d"), {"w": words, "s": [3, 4]})
    got = _load(str(tmp_path / "d"))
    assert set(got) == {"w", "s"} and got["w"].shape == (2, 3)
    assert np.array_equal(got["w"].astype(np.uint64), words) and list(got["s"]) == [3.0, 4.0]
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"a": np.zeros((64 << 20) // 8 + 1, dtype=np.uint64)})
    assert not (tmp_path / "big").exists()


@pytest.mark.parametrize("steps", ["0", "-1"])
def test_steps_below_one_are_refused(steps):
    r = subprocess.run([sys.executable, BENCH, "--steps", steps, "--stub"], env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 2 and b"--steps" in r.stderr, r.stderr.decode()[-2000:]


@pytest.mark.gpu
def test_dump_of_the_cryptonets_batch(tmp_path):
    d = str(tmp_path / "out")
    line = _run("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-unchanged-caller", "--no-single-image", "--no-relinearize-late",
                "--dump-outputs", d)
    assert line["steps"] == 2 and line["verified_against_integer_model"] is True
    got = _load(d)
    primes = (549764251649, 549764284417)
    assert set(got) == {"logit_ciphertexts_p%d" % p for p in primes} | {"logits_mod_p%d" % p for p in primes}
    digest = hashlib.sha256()
    for p in primes:                                       # the words of the verified run, prime after prime: the line's digest
        ct, logits = got["logit_ciphertexts_p%d" % p], got["logits_mod_p%d" % p]
        assert ct.shape == (10, 2, 5, 8192) and logits.shape == (8192, 10)
        assert logits.min() >= 0 and logits.max() < p and np.array_equal(logits, np.rint(logits))
        digest.update(ct.astype(np.uint64).tobytes())
    assert digest.hexdigest() == line["logit_words_sha256"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_full_run_verifies(tmp_path):
    """without --full the line carries the headline alone (no check, no side measurement), and the run computes and dumps what a --full run
    of the same arguments computes and checks against the integer model"""
    plain = _run("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"))
    full = _run("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-unchanged-caller", "--no-single-image", "--no-relinearize-late",
                "--dump-outputs", str(tmp_path / "full"))
    assert plain["full"] is False and full["full"] is True and full["verified_against_integer_model"] is True
    assert not {"verified_against_integer_model", "roofline", "key_switch", "square", "unchanged_caller", "relinearize_late", "cpu_baseline",
                "lola", "cifar"} & set(plain), sorted(plain)
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "logit_words_sha256"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0
    a, b = _load(str(tmp_path / "plain")), _load(str(tmp_path / "full"))
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_dump_of_the_last_lola_image(tmp_path):
    d = str(tmp_path / "out")
    line = _run("--workload", "lola", "--steps", "1", "--warmup", "1", "--no-unchanged-caller", "--dump-outputs", d)
    assert line["steps"] == 1 and line["verified_against_integer_model"] is True
    got = _load(d)
    primes = line["config"]["plaintext_primes"]
    assert set(got) == {"result_ciphertexts_p%d" % p for p in primes} | {"result_slots_mod_p%d" % p for p in primes}
    digest = hashlib.sha256()                              # one timed image: the line's digest covers exactly the dumped words
    for p in primes:
        digest.update(got["result_ciphertexts_p%d" % p].astype(np.uint64).tobytes())
        slots = got["result_slots_mod_p%d" % p]
        assert slots.min() >= 0 and slots.max() < p
    assert digest.hexdigest() == line["result_words_sha256"]
