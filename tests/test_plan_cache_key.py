"""The key and replacement policy of the context's plan cache (csrc/omr_plan_cache.h), on the CPU:
tests/plan_cache_policy_check.cpp replays seeded request streams through plan_cache_key /
plan_cache_find / plan_cache_victim as omr_render.hip does and checks every lookup against a
brute-force LRU list: a hit exactly when the model holds the key (pixel type, bucket count and
plan length are part of it), free slots first, otherwise the least recently used one.  Built here
with g++; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omero-ms-image-region_amd", "csrc")


def test_policy_against_brute_force_model(tmp_path):
    out = str(tmp_path / "plan_cache_policy_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC,
           os.path.join(ROOT, "tests", "plan_cache_policy_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok:")
