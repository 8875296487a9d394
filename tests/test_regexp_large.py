"""Automaton search under every kernel configuration and rank layout.

femto_amd_nfa_search_batch lays the kernel's LDS out by the LARGEST automaton of a batch (tests/regexp_util.lds_plan restates the
host's formulas, nfa_lds_plan in femto_amd/csrc/nfa_batch.hpp; tests/nfa_batch_check.cpp pins the same tuples to the C++) and has one kernel per rank policy and per kLds; tests/test_regexp.py hands it automata of at most 16 nodes and
777 transitions on default handles.  Here:
  * tests/golden/<fixture>_regexp_large.npz (make_regexp_large_golden.py): automata of 24 .. 2048 nodes and up to 13 k
    transitions with the GENUINE do_regexp_query's result lists;
  * CPU: the restatement and the construction against those goldens; that regexp_util.batches reaches every regime a fixture
    can reach, with kLds true and false; that the comparer notices every single corruption; the largest LDS request by hand;
  * GPU: every small and large golden under every configuration on every rank policy, bit for bit; the stack bound, the
    iteration limit and fresh random automata of up to 2048 nodes in those configurations.
Measured on an MI355X: acgt48k and runs3doc 10 configurations per handle (ru, rum, pack, wave), eng2doc 12 (ind, pack2, wave),
bytes256 12 (wave), 100 .. 137 automata per call; a case takes 0.02 .. 1.8 s, on runs3doc's wavelet handle 3.5 .. 4.2 s (its
small list holds one search of 447 k pops); all 128 cases 116 s.  No configuration returned a wrong list."""
import time

import numpy as np
import pytest

import femto_amd
import regexp_util as ru
from oracle import pyoracle as po

FIXTURE_KINDS = [(name, kind) for name in ru.LARGE_FIXTURES for kind in ru.kinds_of(name)]


@pytest.mark.parametrize("name", ru.LARGE_FIXTURES)
def test_fixture_characters(fixtures, name):
    """regexp_util.NCHARS is what the host counts from C[] (nfa_text_chars, nfa_batch.hpp): the documents' bytes and SEOF"""
    fx = fixtures(name)
    o = po.Oracle(fx.index)
    from_c = [c for c in range(261) if o.C(c + 1) > o.C(c)]
    o.close()
    assert from_c == ru.text_chars(fx.docs).tolist() and len(from_c) == ru.NCHARS[name]


def test_lds_plan_by_hand():
    """the four formulas at sizes worked out by hand: acgt48k (5 characters, 8 children) and eng2doc (94 -> 96 children)"""
    P = ru.lds_plan
    assert P(5, 16, 777) == (16, 8, 8, 5, True, "tc")
    assert P(5, 200, 2048)[:5] == (200, 8, 8, 5, True) and P(5, 201, 2049) == (208, 8, 8, 0, False, "group_single")      # 5 * 208 * 4 = 4160 > 4096
    assert P(5, 816, 1) == (816, 8, 5, 0, True, "group_single") and P(5, 817, 1) == (824, 8, 4, 0, True, "group_multi")   # 4096 // 824 = 4 < 5
    assert P(5, 2041, 2040) == (2048, 8, 2, 0, True, "group_multi") and P(5, 2048, 2049) == (2048, 8, 2, 0, False, "group_multi")
    assert P(94, 16, 777) == (16, 96, 64, 0, True, "group_multi") and P(94, 65, 1) == (72, 96, 56, 0, True, "group_multi")
    assert P(94, 1001, 1) == (1008, 96, 4, 0, True, "group_multi") and P(257, 2041, 1) == (2048, 260, 2, 0, True, "group_multi")
    assert P(4, 256, 1) == (256, 4, 4, 4, True, "tc") and P(4, 257, 1) == (264, 4, 4, 0, True, "group_single")          # the text_chars * N * 4 <= 4096 edge
    assert P(64, 16, 1) == (16, 64, 64, 64, True, "tc") and P(65, 16, 1) == (16, 68, 64, 0, True, "group_multi")
    assert P(3, 1, 0) == (8, 4, 4, 3, True, "tc")


def test_largest_lds_request_fits_one_workgroup():
    """The most LDS a launch can ask for: 2048 nodes (lds_group 2), 264 children (261 characters), 2048 transitions in LDS.
    nfa_lds_bytes(2048, 264, 2048, 2) = 8192 (s_tmp) + 264 * 38 = 10032 (the children's arrays) + 6144 (s_cur, s_sub, s_top)
    + 16 + 12288 (s_ent_sd, s_ent_ch) + 2064 (s_flags) + 16400 (s_tmpg) = 55136 bytes of dynamic LDS, plus the kernel's static
    arrays, 4232 bytes: 59368 bytes, under the 65536 one workgroup may have on gfx950 -- hipOccupancyMaxActiveBlocksPerMultiprocessor
    does not answer 0 for it, so nfa_blocks_per_cu's `n < 1` fallback is not what sizes the grid, and B.slots and the `blocks`
    of nfa_arena_plan (nfa_batch.hpp) stay positive.  No other batch asks for more: lds_group * lds_nodes * 4 <= 16384 always, and
    without the transitions in LDS (kLds false) the request is 14352 bytes smaller."""
    assert ru.nfa_lds_bytes(2048, 264, 2048, 2) == 55136 and ru.NFA_STATIC_LDS == 4232
    worst = 0
    for nchars in (1, 5, 64, 65, 94, 257, 261):
        for nodes in list(range(1, 2049, 7)) + [2048]:
            for ents in (0, 2047, 2048, 2049, 1 << 22):
                p = ru.lds_plan(nchars, nodes, ents)
                ne = ((max(ents, 2) + 1) & ~1) if p.klds else 0
                worst = max(worst, ru.nfa_lds_bytes(p.lds_nodes, p.lds_children, ne, p.lds_group))
                assert p.lds_group * p.lds_nodes * 4 <= 16384 or p.lds_group == 1
    assert worst == 55136 and worst + ru.NFA_STATIC_LDS + 16 <= 65536      # (+16: the dynamic array's alignment)


@pytest.mark.parametrize("name", ru.LARGE_FIXTURES)
def test_oracle_restatement_equals_large_goldens(fixtures, name):
    fx = fixtures(name)
    o = po.Oracle(fx.index)
    cases, tags = ru.load_regexp_large_golden(name)
    for (a, rx, approx, want), tag in zip(cases, tags):
        assert ru._same(o.nfa_search(a), want), (name, tag, approx)
    o.close()
    assert len(cases) >= 40 and max(c[0].num_nodes for c in cases) == ru.MAX_NODES


@pytest.mark.parametrize("name", ru.LARGE_FIXTURES)
def test_compiled_automata_equal_the_large_golden_ones(name):
    """the stored pattern texts compile to the stored automata (the reference's lists were produced for exactly these), and the
    named shapes of the issue are all there"""
    cases, tags = ru.load_regexp_large_golden(name)
    n = 0
    for (a, rx, approx, _), tag in zip(cases, tags):
        if rx is None:
            continue
        b = femto_amd.Nfa.from_regex(rx, approx)
        assert b.settings == a.settings and b.num_nodes == a.num_nodes, tag
        for f in ("trans_start", "trans_char", "trans_dest", "is_start", "is_final"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (tag, f)
        n += 1
    size = {t: (c[0].num_nodes, len(c[0].trans_char), c[0].settings) for c, t in zip(cases, tags)}
    for tag, nodes in (("str24", 24), ("str24~1", 24), ("str24~2:1:2:1", 24), ("str251", 251), ("str251~1", 251), ("str1001", 1001),
                       ("str1001~1", 1001), ("str2041", 2041)):
        assert size[tag][0] == nodes and (size[tag][2][0] > 1) == ("~" in tag), (tag, size[tag])
    assert size["str24~2:1:2:1"][2] == (3, 1, 2, 1)
    for tag in ("class220", "class220~1", "class380", "class380~1"):
        assert 200 <= size[tag][0] <= 400, (tag, size[tag])
    for tag in ("wide9", "wide12"):
        assert size[tag][0] <= 24 and size[tag][1] > ru.LDS_ENTS, (tag, size[tag])
    if name == "eng2doc":
        assert 110 <= size["words130"][0] <= 140 and 700 <= size["words760"][0] <= 770 and size["words130~1"][2][0] == 2 and size["words760~1"][2][0] == 2, size
    hand = [(t, s) for t, s in size.items() if t.startswith("hand")]
    for band, (lo, hi) in enumerate(ru.BANDS):
        mine = [s for t, s in hand if t.startswith("hand%d." % band)]
        assert len(mine) >= 6 and all(lo <= s[0] <= hi for s in mine) and {lo, hi} <= {s[0] for s in mine}, (band, mine)
    assert 3 * sum(1 for _, s in hand if s[2][0] > 1) >= len(hand) - 3 and n == len(cases) - len(hand)


# what every fixture's batches must reach: (regime, kLds) pairs, and lds_group values on the byte alphabets.  A regime a fixture
# cannot reach is named here with the reason.
REACH = {
    "acgt48k": {("tc", True), ("tc", False), ("group_single", True), ("group_single", False), ("group_multi", True), ("group_multi", False)},
    "runs3doc": {("tc", True), ("tc", False), ("group_multi", True), ("group_multi", False)},
    "eng2doc": {("group_multi", True), ("group_multi", False)},
    "bytes256": {("group_multi", True), ("group_multi", False)},
}
CANNOT_REACH = {
    "eng2doc": {"tc": "94 characters > 64: lds_tc is 0 for every automaton", "group_single": "94 characters > 64 >= lds_group"},
    "bytes256": {"tc": "257 characters > 64", "group_single": "257 characters > 64 >= lds_group",
                 "ind": "257 characters: no two-level lines, the handle serves the wavelet tree only", "pack2": "as ind"},
}


@pytest.mark.parametrize("name", ru.LARGE_FIXTURES)
def test_batches_reach_every_configuration(name):
    bs = ru.batches(name)
    small = ru.load_regexp_golden(name)
    large, _ = ru.load_regexp_large_golden(name)
    reached = {(b.plan.regime, b.plan.klds) for b in bs}
    assert REACH[name] <= reached, (name, REACH[name] - reached)
    for regime in ("tc", "group_single", "group_multi"):      # what is not reached is named, and really out of reach
        if not any(r == regime for r, _ in reached):
            assert regime in CANNOT_REACH.get(name, {}), (name, regime)
            assert all(ru.lds_plan(ru.NCHARS[name], n, 1).regime != regime for n in range(1, ru.MAX_NODES + 1)), (name, regime)
    for b in bs:      # every batch: the whole small list, and the configuration its key names
        assert b.tags[:len(small)] == ["small"] * len(small) and "small" not in b.tags[len(small):]
        assert all(x[0].num_nodes == y[0].num_nodes and np.array_equal(x[0].trans_dest, y[0].trans_dest) and x[3] is not None for x, y in zip(b.cases, small))
        n, e = max(c[0].num_nodes for c in b.cases), max(len(c[0].trans_char) for c in b.cases)
        assert b.plan == ru.lds_plan(ru.NCHARS[name], n, e) and ru.config_key(b.plan) == b.key
    groups = {b.plan.lds_group for b in bs}
    if ru.NCHARS[name] > 64:
        assert 64 in groups and 2 in groups and any(2 < g <= 8 for g in groups), (name, groups)
    # every large golden is searched in some batch; one batch holds the maximum: >= 2041 nodes with > 2048 transitions
    used = sum(len(b.cases) - len(small) for b in bs)
    assert used >= len(large) and {t for b in bs for t in b.tags} >= set(ru.load_regexp_large_golden(name)[1])
    assert any(max(c[0].num_nodes for c in b.cases) >= 2041 and max(len(c[0].trans_char) for c in b.cases) > ru.LDS_ENTS and not b.plan.klds for b in bs)
    kinds = ru.kinds_of(name)
    assert kinds == {"acgt48k": ["ru", "rum", "pack", "wave"], "runs3doc": ["ru", "rum", "pack", "wave"], "eng2doc": ["ind", "pack2", "wave"], "bytes256": ["wave"]}[name]
    for k in ru.KINDS:
        assert k in kinds or k in CANNOT_REACH.get(name, {}) or not ru.KINDS[k].applies(ru.NCHARS[name])


def test_every_policy_and_klds_is_reached():
    """12 instantiations of nfa_search_kernel: 6 policies x kLds"""
    got = {(ru.KINDS[k].policy, b.plan.klds) for name in ru.LARGE_FIXTURES for k in ru.kinds_of(name) for b in batches_of(name)}
    assert got == {(p, k) for p in ("RuPolicy", "RumPolicy", "PackPolicy", "IndPolicy", "Pack2Policy", "WavePolicy") for k in (True, False)}


def test_comparer_fails_on_each_single_corruption():
    cases = [c for c in ru.load_regexp_golden("acgt48k") if len(c[3][1]) >= 2][:6] + ru.load_regexp_golden("acgt48k")[:10]
    good = ru.answers_of(cases)
    ru.compare_batch(good, cases)
    start, first, last, mlen, cost, status = good
    assert start[1] - start[0] >= 2

    def one(k, at, delta):
        g = [a.copy() for a in good]
        g[k][at] += delta
        return tuple(g)

    def without(at):
        g = [a.copy() for a in good]
        for k in (1, 2, 3, 4):
            g[k] = np.delete(g[k], at)
        g[0][1:] -= 1
        return tuple(g)

    def twice(at):
        g = [a.copy() for a in good]
        for k in (1, 2, 3, 4):
            g[k] = np.insert(g[k], at, g[k][at])
        g[0][1:] += 1
        return tuple(g)

    bad = {"status": one(5, 0, femto_amd.ERR_FULL), "first": one(1, 1, 1), "last": one(2, 1, -1), "length": one(3, 0, 1), "cost": one(4, 1, 1),
           "dropped": without(1), "duplicated": twice(0), "moved": one(0, 1, -1), "last automaton's status": one(5, len(cases) - 1, 1),
           "last result": one(1, len(first) - 1, 1)}
    for what, g in bad.items():
        with pytest.raises(AssertionError):
            ru.compare_batch(g, cases, what)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
_restated, _oracles = {}, {}


def restated(fx, a, **kw):
    """Oracle.nfa_search of one automaton of a fixture, computed once per (automaton, limits)"""
    key = (fx.name, id(a), tuple(sorted(kw.items())))
    if key not in _restated:
        if fx.name not in _oracles:
            _oracles[fx.name] = po.Oracle(fx.index)
        _restated[key] = (a, _oracles[fx.name].nfa_search(a, **kw))      # (keeps `a` alive: its id is the key)
    return _restated[key][1]


_batches = {}


def batches_of(name):
    if name not in _batches:
        _batches[name] = ru.batches(name)
    return _batches[name]


def pick(name, **want):
    """the first batch of a fixture whose plan has the given fields"""
    for b in batches_of(name):
        if all(getattr(b.plan, k) == v for k, v in want.items()):
            return b
    raise AssertionError((name, want, [b.key for b in batches_of(name)]))


def config_id(b):
    return "%s-g%d-%s" % (b.plan.regime, b.plan.lds_group, "lds" if b.plan.klds else "global")


# (one case per batch: a fixture's small list alone takes 0.1 .. 3.5 s per call -- runs3doc's holds a search of 447 k pops)
CONFIGS = [pytest.param(name, kind, k, id="%s-%s-%s" % (name, kind, config_id(b)))
           for name, kind in FIXTURE_KINDS for k, b in enumerate(batches_of(name))]


@pytest.fixture(scope="module")
def kind_handle(fixtures):
    """the handle of (fixture, kind), opened once while consecutive tests ask for the same one, its layout asserted"""
    state = {}

    def get(name, kind):
        if state.get("key") != (name, kind):
            if "ix" in state:
                state.pop("ix").close()
            state["key"] = None
            state["ix"] = ru.open_kind(fixtures(name).index, kind)
            state["key"] = (name, kind)
        return state["ix"]

    yield get
    if "ix" in state:
        state["ix"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,k", CONFIGS)
def test_goldens_under_every_kernel_configuration(fixtures, kind_handle, name, kind, k):
    """every small golden under every configuration, every large golden under its own: one nfa_search_batch call for the batch,
    every automaton's status and four lists bit for bit the genuine reference's"""
    import torch
    assert torch.cuda.is_available()
    ix = kind_handle(name, kind)
    b = batches_of(name)[k]
    t0 = time.time()
    got = ix.nfa_search_batch([c[0] for c in b.cases])
    print("CONFIG %s %s %s lds_nodes=%d lds_group=%d lds_tc=%d klds=%d automata=%d large=%d %.3f s"
          % (name, kind, b.plan.regime, b.plan.lds_nodes, b.plan.lds_group, b.plan.lds_tc, b.plan.klds, len(b.cases), sum(t != "small" for t in b.tags), time.time() - t0))
    ru.compare_batch(got, b.cases, (name, kind, b.key, b.plan))


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [("acgt48k", "ru"), ("acgt48k", "rum"), ("eng2doc", "ind"), ("eng2doc", "pack2")])
def test_stack_retry_under_each_regime(fixtures, name, kind):
    """regexp_stack_cap at its least, 16 pending ranges: in a batch of every regime the fixture has (acgt48k: the by-character
    pass and group_multi; eng2doc, which has no by-character pass: group_multi with lds_group 64 and with lds_group <= 8) some
    search outgrows it and returns ERR_FULL with no results, and every other search returns the restatement's lists; with the
    default bound back the same batches return the unbounded lists.  (A search that outgrows the first arena of 1024 entries
    is then run again in a larger one, `pass > 0`; none of these fixtures' searches needs more than a few hundred entries, so
    here the second part checks that nothing of the first attempt lingers -- scratch buffers, arenas, statuses.)"""
    fx = fixtures(name)
    ix = ru.open_kind(fx.index, kind)
    picks = [pick(name, regime="tc"), pick(name, regime="group_multi")] if ru.NCHARS[name] <= 64 else \
        [pick(name, lds_group=64), next(b for b in batches_of(name) if b.plan.lds_group <= 8 and b.plan.klds)]
    for b in picks:
        ix.set_option("regexp_stack_cap", 16)
        start, first, last, mlen, cost, status = ix.nfa_search_batch([c[0] for c in b.cases])
        full = 0
        for i, c in enumerate(b.cases):
            s, e = int(start[i]), int(start[i + 1])
            if status[i] == femto_amd.ERR_FULL:
                assert e == s, (name, kind, b.key, i)
                full += 1
            else:
                got = (int(status[i]), first[s:e], last[s:e], mlen[s:e], cost[s:e])
                assert ru._same(got, restated(fx, c[0])), (name, kind, b.key, i, b.tags[i], c[1], c[2])
        assert 1 <= full < len(b.cases), (name, kind, b.key, full)
        print("STACK %s %s %s: %d of %d searches ERR_FULL at 16 entries" % (name, kind, b.key, full, len(b.cases)))
        ix.set_option("regexp_stack_cap", 1 << 18)
        ru.compare_batch(ix.nfa_search_batch([c[0] for c in b.cases]), b.cases, (name, kind, b.key, "bound restored"))
    ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind", [("acgt48k", "ru"), ("eng2doc", "ind")])
def test_iteration_limit_under_each_regime(fixtures, name, kind):
    """regexp_max_iterations 3 and 400 on a group_multi batch and on a batch whose transitions stay in global memory (kLds
    false): the GPU and the restatement stop at the same pop (ERR_OVERWORKED, no results) or not at all"""
    fx = fixtures(name)
    ix = ru.open_kind(fx.index, kind)
    picks = [next(b for b in batches_of(name) if b.plan.regime == "group_multi" and b.plan.klds and b.plan.lds_group <= 4), pick(name, regime="tc", klds=False) if ru.NCHARS[name] <= 64 else pick(name, klds=False)]
    for b in picks:
        for limit in (3, 400):
            ix.set_option("regexp_max_iterations", limit)
            got = ix.nfa_search_batch([c[0] for c in b.cases])
            want = [(c[0], c[1], c[2], restated(fx, c[0], max_iterations=limit)) for c in b.cases]
            ru.compare_batch(got, want, (name, kind, b.key, "limit", limit))
            over = int((got[5] == femto_amd.ERR_OVERWORKED).sum())
            assert (over >= 1) if limit == 3 else (over < len(b.cases)), (name, kind, b.key, limit, over)
            print("LIMIT %s %s %s limit %d: %d of %d ERR_OVERWORKED" % (name, kind, b.key, limit, over, len(b.cases)))
    ix.set_option("regexp_max_iterations", 1000000)
    ix.close()


FRESH_SEED = {"acgt48k": 20481, "eng2doc": 20482}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["acgt48k", "eng2doc"])
def test_fresh_large_automata(fixtures, tmp_path, name):
    """300 hand-made automata nobody has searched before, 100 per size band (17..64, 65..512, 513..2048 nodes; every third with
    error costs), one call per band on the default handle: against the restatement, and the first 20 of every band against the
    genuine do_regexp_query where its binary is there"""
    fx = fixtures(name)
    seed = FRESH_SEED[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    alpha = ru.large_alpha(fx.docs)
    ix = femto_amd.Index(fx.index, device=0)
    o = po.Oracle(fx.index)
    for band in range(3):
        nfas = [ru.random_large_nfa(rng, alpha, ru.band_nodes(rng, band, k, 100), approx=k % 3 == 2) for k in range(100)]
        plan = ru.lds_plan(ru.NCHARS[name], max(a.num_nodes for a in nfas), max(len(a.trans_char) for a in nfas))
        got = ix.nfa_search_batch(nfas)
        ru.compare_batch(got, [(a, None, None, o.nfa_search(a)) for a in nfas], (name, "seed", seed, "band", band, plan, "vs restatement"))
        if po.have_ref():
            ref = po.ref_regexp_nfa(fx.index, nfas[:20], str(tmp_path))
            ru.compare_batch(ix.nfa_search_batch(nfas[:20]), [(a, None, None, r) for a, r in zip(nfas[:20], ref)],
                             (name, "seed", seed, "band", band, "vs reference"))
    o.close()
    ix.close()
