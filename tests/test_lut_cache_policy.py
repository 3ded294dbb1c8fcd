"""The eviction policy of the context's device LUT cache (csrc/omr_lut_policy.h), on the CPU:
tests/lut_cache_policy_check.cpp drives lut_cache_victims the way prepare_plan / device_quant_lut
do -- a few thousand seeded plan sequences of 1..32 channels, repeated keys, entry sizes from one
byte to 16 MiB, tiny and large caps -- and checks every answer against a brute-force model: no
entry of the plan being prepared is ever chosen, victims leave least recently used first and no
more of them than the caps ask for, after a plan the cache is within both caps whenever the
plan's own set fits and otherwise holds exactly that set, and the loop ends.  The same program
with the rule the policy replaced (evict the least recently used entry, whoever holds it) must
fail: seventeen 16 MiB LUTs in one plan against the 256 MiB default evict the plan's own first
LUT.  Built here with g++; no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "omero-ms-image-region_amd", "csrc")


@pytest.fixture(scope="module")
def policy_bin(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("lut_policy") / "lut_cache_policy_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC,
           os.path.join(ROOT, "tests", "lut_cache_policy_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_policy_against_brute_force_model(policy_bin):
    r = subprocess.run([policy_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.startswith("ok:")


def test_the_replaced_rule_fails_the_same_check(policy_bin):
    r = subprocess.run([policy_bin, "--old-rule"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1, (r.stdout[-2000:], r.stderr[-2000:])
    assert "17 x 16 MiB in one plan" in r.stdout and "which this plan already holds" in r.stdout
