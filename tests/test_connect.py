"""Conditions on the cases of tests/connect_reference.py, so that tests/test_connect_gpu.py cannot pass by leaving something out: every case has
a finite float64 reference that connects exactly at call num_connect_steps + 1 (a refused case never in its refused calls; its twin after the
counter was at 3 and restarted), the held groups touch nothing during the approach (in float64 and in the checker's float32 build), no threshold
quantity is within 1e-3 of its threshold, env_lookat takes each branch, the slerp each exit and the lift both outcomes, the reference keeps the
invariants of auto-align to 1e-10, and FLOOR is what the float32 build measures now.  No GPU."""
import numpy as np
import pytest

from tests import connect_reference as cr

INVARIANT = 1e-10


@pytest.fixture(scope="module", params=list(cr.MODELS))
def case(request):
    name = request.param
    return dict(name=name, m=cr.model(name), cases=cr.cases(name), refs=cr.reference(name))


@pytest.fixture(scope="module")
def fp32():
    return {name: cr.what_fp32_alone_does(name) for name in cr.MODELS}


def test_no_family_is_empty(case):
    fams = [c["family"] for c in case["cases"]]
    print(case["name"], {f: fams.count(f) for f in cr.FAMILIES[case["name"]]})
    assert set(fams) == set(cr.FAMILIES[case["name"]]) and len(fams) <= 64
    assert {c["group"] for c in case["cases"]} == set(cr.FLOOR[case["name"]])
    assert case["m"].nv <= 30 and case["m"].meta["agent"] == "Cursor"
    # the start state is made of float32 values
    for c in case["cases"]:
        for k in ("qpos", "eq_data", "cursor", "xfrc") + (("twin",) if c["refused"] else ()):
            assert np.array_equal(c[k], c[k].astype(np.float32).astype(np.float64)), k


def test_the_families_hold_what_they_say():
    lack, toy, agne, desk = (cr.cases(n) for n in ("lack", "toy", "agne", "desk"))
    fam = lambda cs, f: [c for c in cs if c["family"] == f]
    # every leg connector against its table connector in both orders over the four angles, with and without a twist of half the forward threshold's angle
    ang = fam(lack, "angles")
    assert {(min(c["k1"], c["k2"]), max(c["k1"], c["k2"])) for c in ang} == {(i, 4 + i) for i in range(4)}
    assert {c["k1"] < 4 for c in ang} == {True, False} and {(min(c["k1"], c["k2"]), c["angle"]) for c in ang} == {(i, a) for i in range(4) for a in (0.0, 90.0, 180.0, 270.0)}
    assert {round(c["twist"] / cr.HALF_FWD) for c in ang} == {-1, 0, 1}
    assert len(fam(lack, "far")) == 8 and all(abs(np.linalg.norm(cr.FAR_AT) - 1.3) < 1e-2 and c["group"] == "far" for c in fam(lack, "far"))
    # no angle list: seven twists, eight orientations each
    free = fam(toy, "free")
    assert all(int(cr.model("toy").conn_nangle[c["k1"]]) == 0 for c in toy)
    for tw in cr.FREE_TWISTS:
        assert sum(1 for c in free if abs(c["twist"]) == tw) >= 8, tw
    # both listed angles of two-angle connectors, and a connector with a single angle
    for cs, name in ((agne, "agne"), (desk, "desk")):
        m = cr.model(name)
        two = [c for c in fam(cs, "two-angle") if int(m.conn_nangle[c["k1"]]) == 2]
        assert {c["angle"] for c in two} == {0.0, 180.0}
    assert any(int(cr.model("desk").conn_nangle[c["k1"]]) == 1 for c in fam(desk, "two-angle"))
    # offsets in both signs; welded groups of 2, 3, 4 parts on either side
    for cs in (lack, toy, agne, desk):
        assert {c["note"] for c in fam(cs, "offsets")} >= {"lateral +1", "lateral -1", "tilt +1", "tilt -1"}
    assert sorted((len(c["members"][1]), len(c["members"][0])) for c in fam(lack, "group")) == [(1, 2), (1, 3), (1, 4), (2, 1), (3, 1), (4, 1)]
    assert all(c["eq_active"].sum() == max(len(c["members"][0]), len(c["members"][1])) - 1 for c in fam(lack, "group"))
    # one refusal per threshold
    for cs, name in ((lack, "lack"), (toy, "toy"), (agne, "agne"), (desk, "desk")):
        want = {"pos", "up", "proj12", "proj21"} | ({"fwd"} if int(cr.model(name).conn_nangle[fam(cs, "refused")[0]["k1"]]) else set())
        assert {c["refused"] for c in fam(cs, "refused")} == want


def test_the_reference_connects_when_it_should(case):
    for e, (c, r) in enumerate(zip(case["cases"], case["refs"])):
        assert cr.finite(r), e
        at = cr.connected_at(r["calls"])
        if c["refused"]:
            # never in the refused calls; the twin approaches three times, the refused pose restarts the counter, the twin then needs all eleven calls
            assert at == [cr.SECOND_CONNECT], (e, c["refused"], at)
            steps = [rec["connect_step"] for rec in r["calls"]]
            assert steps[:cr.CALLS + 1] == [0] * (cr.CALLS + 1) and steps[cr.CALLS + 1:cr.CALLS + 5] == [1, 2, 3, 0], (e, steps)
            assert steps[cr.CALLS + 5:] == list(range(1, cr.NSTEPS + 1)) + [0], (e, steps)
            assert [a["verdict"] for a in r["align"][:cr.CALLS]] == [False] * cr.CALLS and not r["align"][cr.CALLS + 3]["verdict"]
            assert cr.measures(case["m"], c, r, r)["still"] <= INVARIANT  # (the gravity compensation of the start state is a float32 value)
        else:
            assert at == [cr.CALLS], (e, c["family"], c["note"], at)
            assert [rec["connect_step"] for rec in r["calls"][:cr.CALLS + 1]] == list(range(cr.NSTEPS + 1)) + [0]
            last = r["calls"][cr.CALLS]
            assert last["num_connected"] == 1 and last["sel"] == [c["pA"] + 1, 0] and last["roots"][c["pA"]] == last["roots"][c["pB"]]
            assert last["eq_active"].sum() == c["eq_active"].sum() + 1


def test_the_held_groups_touch_nothing_during_the_approach(case, fp32):
    """the masks are only rewritten at the connect: a contact before it would push the parts about, and differently in float32"""
    got = fp32[case["name"]][0]
    for e, (c, r, g) in enumerate(zip(case["cases"], case["refs"], got)):
        upto = cr.ALL_CALLS - 1 if c["refused"] else cr.NSTEPS
        assert cr.touching(case["m"], c, r["calls"], upto) == [], (e, c["family"], c["note"])
        assert cr.touching(case["m"], c, g["calls"], upto) == [], (e, c["family"], c["note"], "float32")


def test_no_threshold_is_a_coin_toss(case):
    """every quantity that an alignment verdict of the reference hangs on is at least MARGIN from its threshold, at every call that asks, and so is
    the condition of the branch that env_lookat takes for the target"""
    low = np.inf
    for e, (c, r) in enumerate(zip(case["cases"], case["refs"])):
        asked = range(len(r["align"])) if c["refused"] else range(cr.CALLS)
        for t in asked:
            a = r["align"][t]
            if a["pos"] == 0.0:  # (a twin that has connected: the sites coincide)
                continue
            clear = min(a["clear"].values())
            low = min(low, clear)
            assert clear >= cr.MARGIN, (e, c["family"], c["refused"], t, a["clear"])
            if a["verdict"]:
                assert a["branch_clear"] >= cr.MARGIN, (e, t, a["branch_clear"])
        if c["refused"]:  # what refuses it is the threshold it is named after, alone
            a = r["align"][0]
            fails = {"pos": a["pos"] >= cr.POS_DIST, "up": a["up"] <= cr.ROT_UP, "fwd": a["fr"] is None, "proj12": a["p12"] <= cr.PROJ, "proj21": a["p21"] <= cr.PROJ}
            assert [k for k, v in fails.items() if v] == [c["refused"]], (e, fails)
            assert c["refused"] not in ("proj12", "proj21") or a["pos"] >= cr.POS_DIST / 2 + cr.MARGIN, (e, a["pos"])  # (nearer than that the projections are not asked)
    print(case["name"], "smallest distance of a deciding quantity from its threshold: %.3e" % low)


def test_the_restated_target_is_the_reference_s(case):
    """alignment() and lookat() of connect_reference restate _is_aligned and lookat_to_quat (they name the branch and the margins): where the reference
    found a pair aligned, its target quaternion is theirs.  The first call's target lays the approach and the last call's is where the connect puts part 2:
    those two are finite in every case (in between, parallel forward vectors may give the reference a NaN target that nothing reads)"""
    for e, (c, r) in enumerate(zip(case["cases"], case["refs"])):
        for t in range(cr.CALLS if not c["refused"] else 0):
            assert r["align"][t]["verdict"]
            target = r["calls"][t + 1]["target"]
            assert np.isfinite(target).all() or 0 < t < cr.CALLS - 1, (e, t)
            if np.isfinite(target).all():
                # (parallel forward vectors: sqrt(1 - cs^2) holds the angle to sqrt(2^-52) = 1.5e-8 rad in float64, whoever computes it)
                assert cr.quat_angle(r["align"][t]["quat"], target) < 1e-7, (e, t)


def test_every_branch_exit_and_lift_outcome_occurs(case):
    refs, cs = case["refs"], case["cases"]
    branches = [r["align"][cr.CALLS - 1]["branch"] for c, r in zip(cs, refs) if not c["refused"]]
    exits = [r["exit"] for c, r in zip(cs, refs) if not c["refused"]]
    lifts = [tuple(r["lift"]) for r in refs if r["lift"]]
    print(case["name"], "branches", [branches.count(b) for b in range(4)], "exits", {x: exits.count(x) for x in set(exits)}, "lifts", lifts)
    assert all(branches.count(b) >= 2 for b in range(4)), branches
    if case["name"] == "lack":
        assert {"same", "flip", "plain"} <= set(exits)
        one = {c["note"]: r for c, r in zip(cs, refs) if c["family"] in ("slerp", "lift")}
        assert one["at the target"]["exit"] == "same" and one["opposite sign"]["exit"] == "flip" and one["twin"]["exit"] == "plain"
        # the 179 degree twist is taken by the allowed angle of 180 degrees, the third of the list
        assert len(one["179 degrees"]["align"][0]["fwd"]) == 3
        # kept: both groups lifted; undone: the table's lifted bounding box leaves the boundary, the leg's does not
        assert one["kept"]["lift"] == [True, True] and one["undone"]["lift"] == [True, False]
        m = case["m"]
        for note, rose in (("kept", (1e-3, 1e-3)), ("undone", (1e-3, 0.0))):
            c = [c for c in cs if c["note"] == note][0]
            r = one[note]
            for p, dz in zip((c["pA"], c["pB"]), rose):  # (the approach moves part 2 alone and the connect puts it 4 cm lower)
                z0, z1 = (cr._part(m, r["calls"][t]["qpos"], p)[0][2] for t in (cr.NSTEPS, cr.CALLS))
                assert abs((z1 - z0) - (dz - (0.004 if p == c["pB"] else 0.0))) < 1e-6, (note, p, z1 - z0)
    else:
        assert not lifts


def test_the_reference_keeps_the_invariants_of_auto_align(case):
    m, low = case["m"], {}
    for e, (c, r) in enumerate(zip(case["cases"], case["refs"])):
        if c["refused"]:
            continue
        v = cr.measures(m, c, r, r)
        s1, s2 = cr.site_pose(m, r["calls"][cr.CALLS]["qpos"], c["k1"])[0], cr.site_pose(m, r["calls"][cr.CALLS]["qpos"], c["k2"])[0]
        gap = float(np.linalg.norm(s2 - s1))
        for k, x in (("site_gap", gap), ("site_ang", v["site_ang"]), ("rigid", v.get("rigid", 0.0))):
            low[k] = max(low.get(k, 0.0), x if not (k == "site_gap" and c["note"] == "undone") else 0.0)
        if c["note"] == "undone":  # the leg went up by the millimetre that the table did not
            assert abs(gap - 1e-3) < 1e-6, gap
        else:
            assert gap <= INVARIANT, (e, gap)
        # (a pre-welded group starts as far from its welds as float32 poses and float32 eq_data are apart, and the welds close that: cr.weld_mismatch)
        assert v["site_ang"] <= INVARIANT and v.get("rigid", 0.0) <= INVARIANT + 2.0 * cr.weld_mismatch(m, c), (e, v, cr.weld_mismatch(m, c))
        assert cr.weld_mismatch(m, c) < 2e-7
        assert set(v) == set(cr.MEASURES) - {"still"} - (set() if max(len(g) for g in c["members"]) > 1 else {"rigid"})
    print(case["name"], "the reference's own", "  ".join("%s %.3e" % kv for kv in low.items()))


def test_what_fp32_alone_does(case, fp32):
    """FLOOR is what a fresh run of the checker's float32 build gives; that build stays finite and takes the reference's decisions in every case"""
    name = case["name"]
    got, fresh = fp32[name]
    for g, d in fresh.items():
        print("%s %s measured: fp32 floor %s" % (name, g, "  ".join("%s %.3e" % kv for kv in d.items())))
    for e, (c, r, g) in enumerate(zip(case["cases"], case["refs"], got)):
        assert cr.finite(g), e
        for t in range(len(r["calls"])):
            assert cr.integers(r["calls"][t]) == cr.integers(g["calls"][t]), (e, c["family"], t)
    assert set(fresh) == set(cr.FLOOR[name])
    for g, d in fresh.items():
        assert set(d) == set(cr.FLOOR[name][g])
        for k, v in d.items():
            assert 0.99 * cr.FLOOR[name][g][k] <= v <= cr.FLOOR[name][g][k], (name, g, k, v, cr.FLOOR[name][g][k])
