"""The receiver batch's device-call dispatcher (asdr_host.cpp) launches every schedule slot exactly once per block.

No GPU: asdr_host.cpp is built with the host compiler against the recording stubs of tools/host_trace_stub.cpp and run through the
scenarios of tools/host_trace_driver.cpp (every launch form: sub-ranges on helper streams, one launch per block, lanes, the block
pipeline with side sub-ranges, SAM and ALS role streams, launch splits, the host path's parts, shards).  The trace names, for every
chain launch, the schedule slots (`sched - d_sched`, `n_sched`) and the blocks (`in_i - dI`, `n_blocks`) it works on.

Per scenario, call and batch (a shard is a batch), with a launch CLASS = (launcher, role, run_if set):
  - no class launches a (slot, block) pair twice;
  - the classes that produce output -- asdr_launch_update_ordered, asdr_launch_update without run_if, asdr_launch_stream, the SAM post role,
    the ALS filter role -- are disjoint and together cover schedule x blocks exactly (one of them alone, for every form but the pipeline
    beside side sub-ranges, where the pipeline and the side launches share the schedule);
  - the other classes cover what their output class covers: SAM pre and PLL = post; the ALS chain (whole, or front and back half) =
    filter; the pipeline's snapshot, restore and gated fallback = the pipeline.
Over the calls of a scenario: the nb_phase / als_phase of a launch equal the blocks issued before it mod 3 / mod 2, and a piece of a
direct group that does not hold the group's first wave never carries lo_write = 1 under the group's own writer bit (ASDR_LO_WRITER).

These are properties of any revision's asdr_host.cpp: ASDR_LAUNCH_PLAN_TREE=<checkout> runs the module against another tree's
include/ and audiosdr_amd/csrc/ (the stubs and the driver stay this tree's)."""
import os
import re
import sys
from collections import Counter

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import host_trace  # noqa: E402

if host_trace.toolchain() is None:
    pytest.skip("no host compiler or no ROCm headers", allow_module_level=True)

with open(os.path.join(ROOT, "tools", "host_trace_driver.cpp")) as _f:
    SCENARIOS = re.findall(r'\{"(\w+)", sc_\w+\}', _f.read())

SLOT_BYTES, BLOCK_BYTES, LO_WRITER = 16, 256, 0x100
CHAIN = ("asdr_launch_update", "asdr_launch_update_ordered", "asdr_launch_sam_role", "asdr_launch_als_role", "asdr_launch_stream", "asdr_launch_stream_snapshot")
OUTPUT = {("asdr_launch_update_ordered", "-", 0), ("asdr_launch_update", "-", 0), ("asdr_launch_stream", "-", 0), ("asdr_launch_sam_role", "2", 0), ("asdr_launch_als_role", "1", 0)}
FOLLOWS = {("asdr_launch_sam_role", "0", 0): ("asdr_launch_sam_role", "2", 0), ("asdr_launch_sam_role", "1", 0): ("asdr_launch_sam_role", "2", 0),
           ("asdr_launch_als_role", "0", 0): ("asdr_launch_als_role", "1", 0), ("asdr_launch_als_role", "2", 0): ("asdr_launch_als_role", "1", 0),
           ("asdr_launch_als_role", "3", 0): ("asdr_launch_als_role", "1", 0),
           ("asdr_launch_stream_snapshot", "snapshot", 0): ("asdr_launch_stream", "-", 0), ("asdr_launch_stream_snapshot", "restore", 0): ("asdr_launch_stream", "-", 0),
           ("asdr_launch_update", "-", 1): ("asdr_launch_stream", "-", 0)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_trace.build(os.environ.get("ASDR_LAUNCH_PLAN_TREE", ROOT), str(tmp_path_factory.mktemp("launch_plan") / "host_trace"))


_parsed = {}


def field(line, name):
    return re.search(r"\b%s=(\S+)" % name, line).group(1)


def dev(text):
    assert text.startswith("dev+"), text
    return int(text[4:], 16)


def calls_of(program, scenario):
    """[(n_blocks, {shard: layout}, [launch])] of a scenario; a launch = dict of the fields the checks read, `base` = its batch's d_sched."""
    if scenario in _parsed:
        return _parsed[scenario]
    bases, calls, cur = [], [], None
    for line in host_trace.run(program, scenario):
        if line.startswith("#call"):
            cur = (int(field(line, "n_blocks")), {}, [])
            calls.append(cur)
        elif line.startswith("#layout"):
            kinds = [int(x) for x in field(line, "kinds").split(",")]
            cur[1][int(field(line, "shard"))] = {"slots": int(field(line, "slots")), "kind_first": [sum(kinds[:k]) for k in range(len(kinds))], "kind_slots": kinds}
        elif line.startswith("asdr_launch_reset"):   # fill_args leaves the schedule's base in it: the first launch of every batch
            if dev(field(line, "sched")) not in bases:
                bases.append(dev(field(line, "sched")))
        elif line.split()[0] in CHAIN and cur is not None:
            name = line.split()[0]
            role = field(line, "role")
            sched = dev(field(line, "sched"))
            base = max(x for x in bases if x <= sched)
            cur[2].append({"cls": (name, "-" if name == "asdr_launch_stream" else role, int(field(line, "run_if"))), "base": base, "shard": bases.index(base),
                           "slot": (sched - base) // SLOT_BYTES, "n_sched": int(field(line, "n_sched")), "in_i": dev(field(line, "in_i")),
                           "n_blocks": int(field(line, "n_blocks")), "nb_phase": int(field(line, "nb_phase")), "als_phase": int(field(line, "als_phase")),
                           "lo_write": int(field(line, "lo_write")), "lo_writer_bit": int(field(line, "lo_writer_bit"), 16), "direct_ch0": int(field(line, "direct_ch0"))})
            assert (sched - base) % SLOT_BYTES == 0
    assert calls and all(c[2] for c in calls), "a call of %s launched nothing" % scenario
    _parsed[scenario] = calls
    return calls


def by_shard(launches):
    out = {}
    for la in launches:
        out.setdefault(la["shard"], []).append(la)
    return out


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_every_slot_of_every_block_is_launched_exactly_once(program, scenario):
    for ci, (n_blocks, layouts, launches) in enumerate(calls_of(program, scenario)):
        groups = by_shard(launches)
        assert sorted(groups) == sorted(layouts), "%s call %d: not every shard launched" % (scenario, ci)
        for shard, group in groups.items():
            where = "%s call %d shard %d" % (scenario, ci, shard)
            d_i = min(la["in_i"] for la in group)
            pairs = {}
            for la in group:
                assert (la["in_i"] - d_i) % BLOCK_BYTES == 0 and la["n_sched"] % 8 == 0 and la["n_sched"] > 0 and la["n_blocks"] > 0, where
                b0 = (la["in_i"] - d_i) // BLOCK_BYTES
                pairs.setdefault(la["cls"], Counter()).update((s, k) for s in range(la["slot"], la["slot"] + la["n_sched"]) for k in range(b0, b0 + la["n_blocks"]))
            for cls, cnt in pairs.items():
                assert cls in OUTPUT or cls in FOLLOWS, "%s: unknown launch class %r" % (where, cls)
                twice = [p for p, c in cnt.items() if c > 1]
                assert not twice, "%s: %r launches (slot, block) %r %d times" % (where, cls, twice[0], cnt[twice[0]])
            total = Counter()
            for cls in pairs:
                if cls in OUTPUT:
                    total.update(pairs[cls])
            want = {(s, k) for s in range(layouts[shard]["slots"]) for k in range(n_blocks)}
            assert set(total) == want and all(c == 1 for c in total.values()), \
                "%s: missing %r, extra %r, twice %r" % (where, sorted(want - set(total))[:3], sorted(set(total) - want)[:3], [p for p, c in total.items() if c > 1][:3])
            for cls in pairs:
                if cls in FOLLOWS:
                    assert FOLLOWS[cls] in pairs and set(pairs[cls]) == set(pairs[FOLLOWS[cls]]), "%s: %r does not cover what %r covers" % (where, cls, FOLLOWS[cls])


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_block_phases_count_the_blocks_issued_before_a_launch(program, scenario):
    before = {}
    for ci, (n_blocks, _, launches) in enumerate(calls_of(program, scenario)):
        for shard, group in by_shard(launches).items():
            d_i = min(la["in_i"] for la in group)
            for la in group:
                issued = before.get(shard, 0) + (la["in_i"] - d_i) // BLOCK_BYTES
                assert (la["nb_phase"], la["als_phase"]) == (issued % 3, issued % 2), \
                    "%s call %d: %r of block %d carries phases %d / %d" % (scenario, ci, la["cls"], issued, la["nb_phase"], la["als_phase"])
            before[shard] = before.get(shard, 0) + n_blocks


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_only_the_piece_with_a_direct_groups_first_wave_writes_its_oscillator_entry(program, scenario):
    for ci, (_, layouts, launches) in enumerate(calls_of(program, scenario)):
        for la in launches:
            if la["direct_ch0"] >= 0 and la["lo_write"] == 1 and la["lo_writer_bit"] == LO_WRITER:
                lay = layouts[la["shard"]]
                firsts = [f for f, s in zip(lay["kind_first"], lay["kind_slots"]) if s > 0]
                assert la["slot"] in firsts, "%s call %d: a piece at slot %d of a direct group writes the oscillator cache" % (scenario, ci, la["slot"])


def test_the_scenarios_reach_the_cases_the_checks_are_about(program):
    """(so that none of the checks above passes for want of launches to look at)"""
    seen, later_pieces = set(), 0
    for scenario in SCENARIOS:
        for _, layouts, launches in calls_of(program, scenario):
            for la in launches:
                seen.add(la["cls"])
                lay = layouts[la["shard"]]
                later_pieces += la["direct_ch0"] >= 0 and la["lo_write"] == 0 and la["lo_writer_bit"] == LO_WRITER and la["slot"] not in lay["kind_first"] and la["cls"][0] == "asdr_launch_update_ordered"
    assert seen == OUTPUT | set(FOLLOWS)
    assert later_pieces > 0
