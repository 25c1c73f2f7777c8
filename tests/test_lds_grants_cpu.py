"""One grant of dynamic LDS per (kernel, device): the bookkeeping every launch above 64 KB goes through
(csrc/swx_common.h::SwxLdsGrants behind swx_lds_grant / swx_launch_lds), checked without a GPU through swx_test_lds_grants, and the
source-level fact that nothing else in csrc/ raises the limit.  The per-process `static bool` guards this replaces forgot that the
attribute belongs to a device's code object, and one of them (a generic lambda's) was shared by four kernels."""
import ctypes
import glob
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNKNOWN, GRANTED, REFUSED = 0, 1, -1
SENTINEL = 77


@pytest.fixture(scope="module")
def grants():
    from stable_ts_amd import _lib
    lib = _lib.load()

    def run(records):
        n = len(records)
        dev = (ctypes.c_int * max(n, 1))(*[d for d, _ in records])
        ok = (ctypes.c_int * max(n, 1))(*[int(o) for _, o in records])
        out = (ctypes.c_int * 64)(*([SENTINEL] * 64))
        return lib.swx_test_lds_grants(dev, ok, n, out), list(out)
    return run


def test_fresh_table_knows_nothing(grants):
    rc, st = grants([])
    assert rc == 0 and st == [UNKNOWN] * 64


def test_a_grant_on_device_0_leaves_the_others_unknown(grants):
    rc, st = grants([(0, True)])
    assert rc == 0 and st[0] == GRANTED and st[1:] == [UNKNOWN] * 63


def test_refusal_and_grant_side_by_side(grants):
    rc, st = grants([(3, False), (5, True)])
    assert rc == 0 and st[3] == REFUSED and st[5] == GRANTED
    assert [s for d, s in enumerate(st) if d not in (3, 5)] == [UNKNOWN] * 62


@pytest.mark.parametrize("ok,want", [(True, GRANTED), (False, REFUSED)])
def test_recording_twice_is_idempotent(grants, ok, want):
    once, twice = grants([(9, ok)]), grants([(9, ok), (9, ok)])
    assert once == twice and once[0] == 0 and once[1][9] == want


def test_first_and_last_device(grants):
    rc, st = grants([(0, False), (63, True)])
    assert rc == 0 and st[0] == REFUSED and st[63] == GRANTED and st[1:63] == [UNKNOWN] * 62
    rc, st = grants([(d, d % 2 == 0) for d in range(64)])
    assert rc == 0 and st == [GRANTED if d % 2 == 0 else REFUSED for d in range(64)]


@pytest.mark.parametrize("dev", [-1, 64, 65, 1 << 20, -(1 << 31)])
def test_device_outside_the_table_is_refused_and_nothing_written(grants, dev):
    for records in ([(dev, True)], [(2, True), (dev, False)], [(dev, True), (2, True)]):
        rc, st = grants(records)
        assert rc == -5 and st == [SENTINEL] * 64, (records, rc)


def test_the_attribute_is_set_in_one_place():
    word = "hipFuncSetAttribute"
    csrc = os.path.join(ROOT, "stable_ts_amd", "csrc")
    holders = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*")) if os.path.isfile(p) and word in open(p, errors="replace").read())
    assert holders == ["swx_common.h"], holders
    hips = glob.glob(os.path.join(csrc, "*.hip"))
    assert len(hips) >= 20 and not [p for p in hips if word in open(p).read()]
    assert sum(word + "(" in ln for ln in open(os.path.join(csrc, "swx_common.h"))) == 1      # one call
