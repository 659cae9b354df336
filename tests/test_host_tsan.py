"""Race detection for the C transport (the reference has none): the lock-free rings, the
futex hand-offs and the rollout slot recycling are stressed under ThreadSanitizer (CPU build only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_transport_stress_is_sanitizer_clean(tmp_path, sanitizer):
    exe = str(tmp_path / "queue_stress")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitizer, "-fno-omit-frame-pointer", "-pthread",
           os.path.join(ROOT, "tests", "native", "queue_stress.cpp"), os.path.join(ROOT, "ga3c_amd", "csrc", "ga3c_host.cpp"),
           "-o", exe, "-lrt"]
    subprocess.check_call(cmd)
    # several copies at once: CPU oversubscription deschedules threads inside the ring's claim/publish windows
    # (this is how the "ring momentarily full behind a descheduled consumer" case was found)
    # ... each with its own GA3C_RESPONDER (include/ga3c_host.h), so that the native loops' helper thread runs here too
    base = {k: v for k, v in os.environ.items() if k != "GA3C_RESPONDER"}
    envs = [base] + [dict(base, GA3C_RESPONDER=mode) for mode in ("1", "2", "3", "2", "1")]
    procs = [subprocess.Popen([exe, "300"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for env in envs]
    for pr in procs:
        out, err = pr.communicate(timeout=240)
        if sanitizer == "thread" and "FATAL: ThreadSanitizer" in err and "unexpected memory mapping" in err:
            pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
        assert pr.returncode == 0, out + err
        assert "WARNING: ThreadSanitizer" not in err and "ERROR: AddressSanitizer" not in err, err
        assert "failures 0" in out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("sanitizer", ["thread", None])
def test_a_herd_of_agents_behind_few_predictors(tmp_path, sanitizer):
    """96 agent threads, the 5 native predictor loops + 4 plain ones: every request answered once with its own values, every
    rollout trained once.  The ring's push is a ticket (fetch_add) since a compare-and-swap loop collapsed under such herds
    (profiles/README.md); this holds it to the same invariants as the small case, with and without ThreadSanitizer."""
    exe = str(tmp_path / "queue_herd")
    cmd = ["g++", "-std=c++17", "-O2" if sanitizer is None else "-O1", "-g", "-pthread"]
    if sanitizer:
        cmd += ["-fsanitize=" + sanitizer, "-fno-omit-frame-pointer"]
    cmd += [os.path.join(ROOT, "tests", "native", "queue_stress.cpp"), os.path.join(ROOT, "ga3c_amd", "csrc", "ga3c_host.cpp"),
            "-o", exe, "-lrt"]
    subprocess.check_call(cmd)
    pr = subprocess.run([exe, "200" if sanitizer is None else "60", "96", "4"], capture_output=True, text=True, timeout=240)
    if sanitizer == "thread" and "FATAL: ThreadSanitizer" in pr.stderr and "unexpected memory mapping" in pr.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory in this container")
    assert pr.returncode == 0, pr.stdout + pr.stderr
    assert "WARNING: ThreadSanitizer" not in pr.stderr, pr.stderr
    assert "failures 0" in pr.stdout
