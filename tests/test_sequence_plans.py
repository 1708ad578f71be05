"""CPU check, with the oracle alone, that the sequence fuzz of
tests/test_gpu_sequences.py cannot pass vacuously: its 32 plans really carry
matches from one stream of a context to a later one, reach the fused index
insert, grow a context's tables steeply and take every path often.  The counts
are pinned: a change of the plan generator (tests/seq_model.py) that moves them
shows here, on a machine without a GPU."""
from collections import Counter

import pytest

from oracle import oracle
from tests import seq_model as sm

NPLANS = 32  # the plans the GPU test runs by default


@pytest.fixture(scope="module")
def plans():
    oracle.build()
    out = []
    for seed in range(NPLANS):
        plan = sm.make_plan(seed)
        for st in plan["steps"]:  # (the sizes are all these tests need of the streams)
            st["n"] = int(st.pop("data").size)
        out.append((plan, sm.plan_records(seed)))
    return out


def test_plans_are_reproducible_and_within_the_shapes(plans):
    one, two = sm.make_plan(5), sm.make_plan(5)
    assert sm.describe(one) == sm.describe(two)
    assert all((a["data"] == b["data"]).all() for a, b in zip(one["steps"], two["steps"]))
    assert [st["data"].size for st in one["steps"]] == [st["n"] for st in plans[5][0]["steps"]]
    for plan, _ in plans:
        assert plan["W"] in sm.WS and 6 <= len(plan["steps"]) <= 10
        assert all(st["n"] < (6 << 20) + plan["W"] for st in plan["steps"])
    assert {plan["W"] for plan, _ in plans} == set(sm.WS)
    assert sum(1 for plan, _ in plans if plan["seeds"]) == 11  # a third: seeded from another stream's chunks
    assert sum(1 for plan, _ in plans if plan["sha1"]) == 24


def test_every_sha1_plan_matches_a_chunk_of_an_earlier_stream(plans):
    """A D record whose match is a chunk an earlier stream of the context saved:
    its id is in the carried index only, and the oracle run with the carried
    index empty does not report it as a duplicate."""
    missing = [plan["seed"] for plan, out in plans if plan["sha1"] and not any(o["carried"] for o in out)]
    assert missing == []
    # and a context without ZC_FLAG_SHA1 carries nothing
    assert all(o["added"] == 0 for plan, out in plans if not plan["sha1"] for o in out)


def test_plans_reach_the_fused_insert_steep_growth_and_every_path(plans):
    fused, steep, paths, lengths = 0, 0, Counter(), Counter()
    for plan, out in plans:
        W = plan["W"]
        ns = [st["n"] for st in plan["steps"]]
        # predicted fused: the model's restatement of the condition, on tables
        # no larger than an earlier whole-stream epoch of the context made
        fused += any(o["fused"] and o["fits"] for o in out)
        # small -> large: n / W grows 64-fold or more from one stream to the next
        steep += any(ns[i] >= 64 * max(ns[i - 1], 1) and ns[i] // W >= 64 for i in range(1, len(ns)))
        paths.update(st["path"] for st in plan["steps"])
        for n in ns:
            lengths["0/1" if n <= 1 else "W+-1" if n in (W - 1, W + 1) else
                    "tiles" if n % sm.STILE in (0, W - 1) else "uniform"] += 1
    assert (fused, steep) == (11, 21)
    assert fused >= 8 and steep >= 8
    assert paths == {"device": 68, "host": 66, "window": 63, "feed0": 60}
    assert min(paths.values()) >= 20
    assert all(lengths[k] >= 10 for k in ("0/1", "W+-1", "tiles", "uniform")), lengths
