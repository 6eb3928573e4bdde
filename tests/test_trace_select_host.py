"""Which instantiation of the closest-hit kernel (K2) and of the shadow-ray kernel (K3) a launch takes (ray_amd/csrc/trace_select.h), checked on
the host over the whole table.

tests/hostsim/trace_select_check.cpp is a stand-alone program over trace_select.h -- the header the passes, the kernel-level hooks and the
reports (rayhip_closest_hit_form, rayhip_direct_entry) share.  It prints the form closest_form / shadow_form name for every combination of
BVH width, role (primary / secondary pass, hook), count flags, RAYHIP_REFILL, pool_scene, small_scene, direct, shadow_refill, hook_refill and the
two wave-count knobs.  The rules below are written out here, not taken from the header: the priority list of a pass, the table by
RAYHIP_REFILL, every difference between a pass and a hook, and what must hold of the table as a whole."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "trace_select_check.cpp")

K2_FORMS = {"counted8", "counted4", "counted0", "plain8", "plain8small", "plain4", "plain4small", "plain0", "whole8", "whole4", "whole4direct",
            "lane8", "lane4", "lane4direct", "pooled"}
K3_FORMS = {"counted8", "counted4", "counted0", "plain8", "plain8small", "plain4", "plain4small", "plain0", "refill", "refilldirect"}
INT_KEYS = ("wide", "cw", "ct", "refill", "pool", "small", "direct", "srefill", "hrefill", "pw", "sw")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("trace_select") / "trace_select_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    rows = []
    for line in r.stdout.splitlines():
        w = line.split()
        row = dict(zip(w[0::2], w[1::2]))
        for k in INT_KEYS:
            row[k] = int(row[k])
        rows.append(row)
    return rows


def refill_family(wide, direct, kind):
    """the refill forms of a width: 8, 4-direct or 4"""
    return kind + ("8" if wide == 8 else "4direct" if direct else "4")


def plain_family(wide, small):
    return "plain0" if wide == 0 else "plain%d%s" % (wide, "small" if small else "")


def expect_k2(r):
    wide, hook, primary = r["wide"], r["role"] == "hook", r["role"] == "primary"
    refill_on = r["refill"] != 0
    whole = r["refill"] in (3, 4)            # refill_primary_whole
    secondary_only = r["refill"] in (2, 3, 4)  # refill_secondary_only
    pooled = wide == 4 and r["refill"] == 4 and r["pool"]
    # 1. COUNT_WIDE and a wide tree; 2. COUNT_TRAVERSAL: without COUNT_WIDE in a pass, the raw bit in the hook
    if r["cw"] and wide in (4, 8):
        return "counted%d" % wide
    if r["ct"] and (hook or not r["cw"]):
        return "counted0"
    if hook:
        if pooled:
            return "pooled"
        if wide and refill_on:
            return refill_family(wide, r["direct"], "lane")
        return plain_family(wide, False)  # never the small forms
    if wide and refill_on and whole and primary:  # 3.
        return refill_family(wide, r["direct"], "whole")
    if pooled and not primary:  # 4.
        return "pooled"
    if wide and refill_on and not (secondary_only and primary):  # 5.
        return refill_family(wide, r["direct"], "lane")
    return plain_family(wide, r["small"] or r["pw"] == 5)  # 6.


def expect_k3(r):
    wide = r["wide"]
    if r["role"] == "hook":
        if r["hrefill"] and wide == 4:
            return "refilldirect" if r["direct"] else "refill"
        return "counted0"
    if r["cw"] and wide in (4, 8):
        return "counted%d" % wide
    if r["ct"] and not r["cw"]:
        return "counted0"
    if wide == 4 and r["srefill"]:
        return "refilldirect" if r["direct"] else "refill"
    return plain_family(wide, r["small"] or r["sw"] == 5)


def test_table_is_complete(table):
    """every combination once: 3 widths (direct doubles width 4) x 3 roles x 4 flag pairs x 5 refill modes x 2^6 remaining switches"""
    assert len(table) == (3 + 1) * 3 * 4 * 5 * 64
    keys = {tuple(r[k] for k in INT_KEYS) + (r["role"],) for r in table}
    assert len(keys) == len(table)
    assert {r["k2"] for r in table} <= K2_FORMS and {r["k3"] for r in table} <= K3_FORMS


def test_priority_lists(table):
    bad = [r for r in table if r["k2"] != expect_k2(r) or r["k3"] != expect_k3(r)]
    assert not bad, (len(bad), bad[0], expect_k2(bad[0]), expect_k3(bad[0]))


def test_table_by_refill_mode(table):
    """a 4-wide scene without count flags, neither small nor tuned: RAYHIP_REFILL against primary / secondary"""
    want = {0: ("plain", "plain"), 1: ("lane", "lane"), 2: ("plain", "lane"), 3: ("whole", "lane"), 4: ("whole", "pooled-or-lane")}
    seen = 0
    for r in table:
        if r["wide"] != 4 or r["cw"] or r["ct"] or r["small"] or r["pw"] or r["role"] == "hook":
            continue
        kind = want[r["refill"]][0 if r["role"] == "primary" else 1]
        if kind == "pooled-or-lane":
            kind = "pooled" if r["pool"] else "lane"
        expect = {"plain": "plain4", "pooled": "pooled"}.get(kind, kind + ("4direct" if r["direct"] else "4"))
        assert r["k2"] == expect, r
        seen += 1
    assert seen == 2 * 5 * 2 * 2 * 2 * 2 * 2  # roles x modes x pool x direct x srefill x hrefill x sw


def by_key(table, role):
    return {tuple(r[k] for k in INT_KEYS): r for r in table if r["role"] == role}


def test_pass_and_hook_differences(table):
    prim, sec, hook = by_key(table, "primary"), by_key(table, "secondary"), by_key(table, "hook")
    met = {k: 0 for k in ("raw_count_bit", "whole", "secondary_only", "small", "pooled_primary", "k3")}
    for key, h in hook.items():
        p, s = prim[key], sec[key]
        # COUNT_WIDE | COUNT_TRAVERSAL on a BVH2 scene: counted in the hook, plain in a pass
        if h["wide"] == 0 and h["cw"] and h["ct"]:
            assert h["k2"] == "counted0" and p["k2"] == s["k2"] == "plain0"
            met["raw_count_bit"] += 1
        if h["cw"] or h["ct"]:
            continue
        # the hook never takes its chunks whole, whatever refill_primary_whole says ...
        assert not h["k2"].startswith("whole")
        if p["k2"].startswith("whole"):
            assert h["k2"] == "pooled" or h["k2"] == p["k2"].replace("whole", "lane")
            met["whole"] += 1
        # ... ignores refill_secondary_only ...
        if h["refill"] == 2 and h["wide"]:
            assert p["k2"].startswith("plain") and h["k2"].startswith("lane")
            met["secondary_only"] += 1
        # ... and small_scene / RAYHIP_PRIMARY_WAVES
        assert not h["k2"].endswith("small")
        if p["k2"].endswith("small"):
            assert h["k2"] + "small" == p["k2"] or h["refill"] == 2
            met["small"] += 1
        # the hook pools although it launches with init_hits == 0, which a pass never does
        assert p["k2"] != "pooled"
        if h["k2"] == "pooled":
            assert s["k2"] == "pooled"
            met["pooled_primary"] += 1
        # beyond that the hook launches what the secondary bounces of a pass launch, up to the small forms
        assert h["k2"] == s["k2"] or h["k2"] + "small" == s["k2"], (h, s)
    for key, h in hook.items():
        # K3: the persistent form on request only (whatever shadow_refill says), otherwise the instrumented BVH2 walk whatever width and flags
        assert h["k3"] == (("refilldirect" if h["direct"] else "refill") if h["hrefill"] and h["wide"] == 4 else "counted0")
        if h["k3"] != prim[key]["k3"]:
            met["k3"] += 1
        assert prim[key]["k3"] == sec[key]["k3"]  # (a pass: one K3 rule for every bounce)
    assert all(met.values()), met


def test_direct_forms_replace_4_wide_refill_forms_only(table):
    for r in table:
        for k in ("k2", "k3"):
            if r[k].endswith("direct"):
                assert r["direct"] and r["wide"] == 4, r
            elif r["direct"]:
                assert r[k] not in ("whole4", "lane4", "refill"), r
    # ... and switching `direct` changes nothing else
    with_direct = {tuple(r[k] for k in INT_KEYS if k != "direct") + (r["role"],): r for r in table if r["direct"]}
    for r in table:
        if r["wide"] == 4 and not r["direct"]:
            d = with_direct[tuple(r[k] for k in INT_KEYS if k != "direct") + (r["role"],)]
            for k in ("k2", "k3"):
                assert d[k] == (r[k] + "direct" if r[k] in ("whole4", "lane4", "refill") else r[k]), (r, d)


def test_every_form_is_reachable(table):
    assert {r["k2"] for r in table} == K2_FORMS
    assert {r["k3"] for r in table} == K3_FORMS
    # ... and by a pass (the hooks add no form of their own)
    assert {r["k2"] for r in table if r["role"] != "hook"} == K2_FORMS
    assert {r["k3"] for r in table if r["role"] != "hook"} == K3_FORMS


def test_width_0_takes_the_bvh2_forms(table):
    for r in table:
        if r["wide"] == 0:
            assert r["k2"] in ("plain0", "counted0") and r["k3"] in ("plain0", "counted0"), r


def test_k3_small_is_the_default(table):
    """RAYHIP_SHADOW_WAVES defaults to 5: a pass without the persistent form takes the small nested form"""
    for r in table:
        if r["role"] != "hook" and not r["cw"] and not r["ct"] and r["wide"] and not (r["wide"] == 4 and r["srefill"]):
            assert r["k3"].endswith("small") == bool(r["small"] or r["sw"] == 5), r
