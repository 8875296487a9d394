"""Plain-Python helpers of the automaton-search tests (tests/test_regexp.py, tests/test_regexp_large.py); no GPU here.

  * the loader of tests/golden/<fixture>_regexp.npz and <fixture>_regexp_large.npz and the comparer of result lists,
  * lds_plan: the host's choice of the kernel's LDS layout, restated,
  * KINDS: the handle options behind every rank policy nfa_search_kernel is instantiated for,
  * batches: for a fixture, one batch of automata per kernel configuration its goldens can reach,
  * random_large_nfa: hand-made acyclic automata of 17..2048 nodes (the golden generator's and the fresh ones of the GPU test)."""
import os
from collections import namedtuple

import numpy as np

import femto_amd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LARGE_FIXTURES = ["acgt48k", "eng2doc", "bytes256", "runs3doc"]
SEOF = 2
MAX_NODES = 2048            # what femto_amd_nfa_search_batch accepts (validate_nfa)
LDS_ENTS = 2048             # kNfaLdsEnts: up to this many transitions the automaton itself is copied to LDS


def load_regexp_golden(name, suffix="_regexp"):
    """[(Nfa, regex bytes or None, approx tuple, (err_code, first, last, len, cost))] of one fixture"""
    g = np.load(os.path.join(GOLDEN, name + suffix + ".npz"))
    out, ts, tt, tn, rr = [], 0, 0, 0, 0
    for i in range(int(g["n"])):
        n = int(g["num_nodes"][i])
        tstart = g["trans_start"][ts:ts + n + 1]
        t = int(tstart[-1])
        a = femto_amd.Nfa(tstart, g["trans_char"][tt:tt + t], g["trans_dest"][tt:tt + t], g["is_start"][tn:tn + n],
                          g["is_final"][tn:tn + n], tuple(int(v) for v in g["settings"][i]))
        c = int(g["res_count"][i])
        want = (int(g["err_code"][i]), g["res_first"][rr:rr + c], g["res_last"][rr:rr + c], g["res_len"][rr:rr + c], g["res_cost"][rr:rr + c])
        out.append((a, bytes(g["regex"][i]) if g["from_regex"][i] else None, tuple(int(v) for v in g["approx"][i]), want))
        ts += n + 1
        tt += t
        tn += n
        rr += c
    return out


def load_regexp_large_golden(name):
    """the same tuples from <name>_regexp_large.npz (tests/golden/make_regexp_large_golden.py), and the name of every automaton"""
    g = np.load(os.path.join(GOLDEN, name + "_regexp_large.npz"))
    return load_regexp_golden(name, "_regexp_large"), [bytes(t).decode() for t in g["tag"]]


def _same(got, want):
    return got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))


def text_chars(docs):
    """alpha codes the text of a fixture holds: its bytes + 5 and SEOF, which ends every document (Fixture.prepared_text);
    their number is what the host counts from C[] (nfa_text_chars, femto_amd/csrc/nfa_batch.hpp)"""
    return np.concatenate([[SEOF], np.unique(np.concatenate(docs)).astype(np.int32) + 5]).astype(np.int32)


# ---- the kernel's configuration -------------------------------------------------------------------------------------------
Plan = namedtuple("Plan", "lds_nodes lds_children lds_group lds_tc klds regime")


def lds_plan(nchars, max_nodes, max_ents):
    """femto_amd_nfa_search_batch's LDS layout for a batch (nfa_lds_plan, femto_amd/csrc/nfa_batch.hpp: lds_nodes, lds_children,
    lds_ents / kLds, lds_group, lds_tc; tests/nfa_batch_check.cpp pins the same tuples to the C++): nchars = characters the text
    holds, max_nodes / max_ents = the batch's largest node and transition counts.  The regime is what the child phase of a pop
    then does: "tc" the by-character pass (lds_tc > 0), "group_single" every live child in one group (nfa_search_kernel's loop
    over the groups of live children, the one that counts `g0`, runs once), "group_multi" more live children than a group holds
    (that loop with g0 > 0)."""
    lds_nodes = (max(int(max_nodes), 1) + 7) & ~7
    lds_children = (max(int(nchars), 4) + 3) & ~3
    lds_group = max(1, min(lds_children, 64, 16384 // (lds_nodes * 4)))
    lds_tc = nchars if (nchars <= 64 and nchars <= lds_group and nchars * lds_nodes * 4 <= 4096) else 0
    klds = int(max_ents) <= LDS_ENTS
    regime = "tc" if lds_tc else ("group_multi" if (lds_group < nchars or nchars > 64) else "group_single")
    return Plan(lds_nodes, lds_children, lds_group, lds_tc, klds, regime)


def nfa_lds_bytes(nn, cc, ne, group):
    """dynamic LDS of one workgroup, restated from nfa_lds_bytes (femto_amd/csrc/nfa_batch.hpp)"""
    return nn * 4 + cc * (8 + 8 + 4 + 4 + 4 + 4 + 4 + 2) + nn * 3 + 16 + ne * 6 + ((nn + 16) if ne else 0) + ((group * nn * 4 + 16) if group else 0)


# the static __shared__ arrays of nfa_search_kernel (regexp_search.hip): s_bychar i32[264], s_text u32[9], s_code u16[264],
# s_textch u16[264], s_alive u8[264], s_textpos u8[264], s_q i32, s_pend u32[256], s_char_child i16[264]
NFA_STATIC_LDS = 264 * 4 + 9 * 4 + 264 * 2 + 264 * 2 + 264 + 264 + 4 + 256 * 4 + 264 * 2


# ---- the rank policies ----------------------------------------------------------------------------------------------------
# name -> (policy, handle options, the alphabets it exists for, a predicate on the open handle that proves the layout)
Kind = namedtuple("Kind", "policy options applies proves")


def _pi(ix):
    return ix.pack_info()


_small = lambda nchars: nchars <= 8              # the packed 3-bit lines (mode 3)
_bytes = lambda nchars: 9 <= nchars <= 256        # the two-level lines (mode 4)
KINDS = {
    "ru": Kind("RuPolicy", None, _small, lambda ix: ix.rank_mode == 3 and _pi(ix)["rank_units"] and not _pi(ix)["rank_units_marked"]),
    "rum": Kind("RumPolicy", dict(rank_units=3, dense_arrays=0, text=0), _small,
                lambda ix: ix.rank_mode == 3 and _pi(ix)["rank_units"] and _pi(ix)["rank_units_marked"]),
    "pack": Kind("PackPolicy", dict(rank_units=0), _small, lambda ix: ix.rank_mode == 3 and not _pi(ix)["rank_units"]),
    "ind": Kind("IndPolicy", None, _bytes, lambda ix: ix.rank_mode == 4 and _pi(ix)["char_rank_lines"]),
    "pack2": Kind("Pack2Policy", dict(char_rank_lines=0), _bytes, lambda ix: ix.rank_mode == 4 and not _pi(ix)["char_rank_lines"]),
    "wave": Kind("WavePolicy", dict(rank_mode=1), lambda nchars: True, lambda ix: ix.rank_mode == 1),
}
# characters of the large-golden fixtures' texts (test_regexp_large.py checks them against the documents)
NCHARS = {"acgt48k": 5, "eng2doc": 94, "bytes256": 257, "runs3doc": 5}


def kinds_of(name):
    return [k for k, v in KINDS.items() if v.applies(NCHARS[name])]


def open_kind(path, kind):
    """the handle of one kind on GPU 0, its layout asserted"""
    ix = femto_amd.Index(path, device=0, options=KINDS[kind].options)
    assert KINDS[kind].proves(ix), (kind, ix.rank_mode, ix.pack_info())
    return ix


# ---- batches --------------------------------------------------------------------------------------------------------------
Batch = namedtuple("Batch", "key plan cases tags")


def group_class(lds_group):
    """lds_group by powers of two: 64, 32 (32..63), 16, 8, 4, 2, 1"""
    return 1 << (int(lds_group).bit_length() - 1)


def config_key(plan):
    return (plan.regime, group_class(plan.lds_group), plan.klds)


def _size(case):
    return case[0].num_nodes, len(case[0].trans_char)


def batches(name, nchars=None):
    """One Batch per kernel configuration -- (regime, lds_group by powers of two, kLds) -- that the fixture's goldens reach.
    Every batch is the fixture's WHOLE small golden list plus large goldens that move the batch's maxima into that
    configuration: every large golden goes into the batch of the configuration it reaches on top of the small list alone (so
    each is searched once per handle), and a configuration that only two large goldens together reach -- one with the nodes,
    one with the transitions -- gets a batch of the small list and the cheapest such pair."""
    nchars = NCHARS[name] if nchars is None else nchars
    small = load_regexp_golden(name)
    large, tags = load_regexp_large_golden(name)
    n0 = max(_size(c)[0] for c in small)
    e0 = max(_size(c)[1] for c in small)
    plan0 = lds_plan(nchars, n0, e0)
    members = {config_key(plan0): []}
    for i, c in enumerate(large):
        n, e = _size(c)
        members.setdefault(config_key(lds_plan(nchars, max(n0, n), max(e0, e))), []).append(i)
    pairs = {}
    for i in range(len(large)):
        for j in range(i + 1, len(large)):
            (ni, ei), (nj, ej) = _size(large[i]), _size(large[j])
            key = config_key(lds_plan(nchars, max(n0, ni, nj), max(e0, ei, ej)))
            cost = ni * ei + nj * ej
            if key not in members and (key not in pairs or cost < pairs[key][0]):
                pairs[key] = (cost, [i, j])
    for key, (_, ij) in pairs.items():
        members[key] = ij
    out = []
    for key in sorted(members, key=lambda k: (k[0], -k[1], not k[2])):
        idx = members[key]
        cases = small + [large[i] for i in idx]
        plan = lds_plan(nchars, max(_size(c)[0] for c in cases), max(_size(c)[1] for c in cases))
        assert config_key(plan) == key, (name, key, plan)
        out.append(Batch(key, plan, cases, ["small"] * len(small) + [tags[i] for i in idx]))
    return out


# ---- hand-made automata ---------------------------------------------------------------------------------------------------
BANDS = [(17, 64), (65, 512), (513, 2048)]


def large_alpha(docs):
    """what random_large_nfa draws transitions from: characters of the text (twice: most transitions can be followed), SEOF and
    one character the text lacks; of a byte text only its eight most frequent characters (a random byte seldom follows another)"""
    flat = np.concatenate(docs)
    count = np.bincount(flat, minlength=256)
    have = np.flatnonzero(count)
    lacks = [c + 5 for c in range(256) if count[c] == 0][:1] or [1]       # (a full byte alphabet: EOF's neighbour, never in a text)
    if len(have) > 16:
        have = np.sort(np.argsort(-count, kind="stable")[:8])
    chars = have.astype(np.int32) + 5
    return np.concatenate([chars, chars, np.array([SEOF] + lacks, dtype=np.int32)])


def random_large_nfa(rng, alpha, nodes, approx):
    """An acyclic automaton in the style of make_regexp_golden.random_nfa with `nodes` nodes: 1..4 transitions per node to
    later nodes anywhere up to the last (so the alive states spread over all node indices), a few start states besides node
    0, final states thin enough that a search reads several characters.  Every non-final node has a transition and
    insert_cost <= subst_cost (the reference waits for ever otherwise, see random_nfa)."""
    n = int(nodes)
    per = np.concatenate([rng.integers(1, 5, size=n - 1), [0]])
    ts = np.concatenate([[0], np.cumsum(per)])
    src = np.repeat(np.arange(n), per)
    tc = np.asarray(alpha)[rng.integers(0, len(alpha), size=len(src))]
    td = src + 1 + np.floor(rng.random(len(src)) * (n - 1 - src)).astype(np.int64)
    st = np.zeros(n, dtype=np.uint8)
    st[0] = 1
    st[rng.integers(0, n - 1, size=int(rng.integers(0, 4)))] = 1
    fi = (rng.random(n) < float(rng.choice([0.02, 0.05, 0.2]))).astype(np.uint8)
    fi[st == 1] = 0                     # (a final start state: the whole index is the one result, nothing is searched)
    fi[n - 1] = 1
    se = (1, 1, 1, 1)
    if approx:
        b = int(rng.integers(2, 4))
        ins = max(int(rng.integers(1, 3)), (b + 2) // 3)
        se = (b, max(int(rng.integers(1, 3)), ins), int(rng.integers(1, 3)), ins)
    return femto_amd.Nfa(ts, tc, td, st, fi, se)


def band_nodes(rng, band, k, count):
    """node counts for the k-th of `count` automata of a band: its two ends first, then random sizes inside it"""
    lo, hi = BANDS[band]
    return lo if k == 0 else (hi if k == 1 else int(rng.integers(lo, hi + 1)))


# ---- comparing -------------------------------------------------------------------------------------------------------------
def answers_of(cases):
    """what nfa_search_batch owes for `cases`, in its own form: (result_start, first, last, match_len, cost, status)"""
    want = [c[3] for c in cases]
    start = np.concatenate([[0], np.cumsum([len(w[1]) for w in want])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(w[k], dtype=dt) for w in want]) if want else np.zeros(0, dtype=dt)
    return start, cat(1, np.int64), cat(2, np.int64), cat(3, np.int32), cat(4, np.int32), np.array([w[0] for w in want], dtype=np.int32)


def compare_batch(got, cases, what=()):
    """The one comparison of a batch's answer (pure numpy): every automaton's status and four lists, bit for bit"""
    start, first, last, mlen, cost, status = got
    what = what if isinstance(what, tuple) else (what,)
    assert len(status) == len(cases) and len(start) == len(cases) + 1, ("lengths", len(status), len(start), len(cases)) + what
    assert start[0] == 0 and start[-1] == len(first) == len(last) == len(mlen) == len(cost), ("total", int(start[-1]), len(first)) + what
    for i, (a, rx, approx, want) in enumerate(cases):
        s, e = int(start[i]), int(start[i + 1])
        g = (int(status[i]), first[s:e], last[s:e], mlen[s:e], cost[s:e])
        assert _same(g, want), what + (i, (rx or b"")[:40], approx, a.num_nodes, len(a.trans_char), a.settings, "status", g[0], want[0], "results", e - s, len(want[1]))
