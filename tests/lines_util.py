"""Test helper: the rule of include/femto_amd.h "matching lines" (print_grep, src/main_cc/search_tool.cc:278-351, over the
document's bytes) restated twice -- (a) the literal loops over one document's bytes, (b) vectorised with searchsorted over
the positions of the stop bytes -- plus the grouping of equal lines in numpy and the output of the search tool's --lines /
--multilines as python formats it."""
import numpy as np

MAX_LINE = 1024
BINARY, INVALID = 1, 2
FIXTURES = ["acgt48k", "b1000", "bytes256", "chunks2doc", "counter400_default", "counter400_small", "eng2doc", "runs3doc",
            "construct_kat"]


# (a)
def line_loops(b, o):
    """(line_start, line_len, binary) for the anchor at offset o of the document with bytes b (0 <= o <= len(b))"""
    L = len(b)
    start = end = o
    binary = False
    i = 1
    while i < MAX_LINE:
        if o - i < 0 or o - i >= L:
            break
        c = b[o - i]
        if c == 10 or c == 13:
            break
        if c == 0:
            binary = True
            break
        start = o - i
        i += 1
    if i == MAX_LINE:
        binary = True
    i = 0
    while i < MAX_LINE:
        if o + i >= L:
            break
        end = o + i
        c = b[o + i]
        if c == 10 or c == 13:
            break
        if c == 0:
            binary = True
            break
        i += 1
    if i == MAX_LINE:
        binary = True
    return start, end - start, binary


# (b)
def lines_of_document(b, o):
    """line_loops for an array of offsets o into the document b, vectorised: (start, len, binary) arrays"""
    b = np.asarray(b, dtype=np.uint8)
    o = np.asarray(o, dtype=np.int64)
    L = len(b)
    stops = np.nonzero((b == 10) | (b == 13) | (b == 0))[0].astype(np.int64)
    # backward: the last stop in [max(0, o - 1023), o)
    k = np.searchsorted(stops, o, side="left") - 1
    prev = np.where(k >= 0, stops[np.maximum(k, 0)] if len(stops) else -1, -1)
    lo = np.maximum(o - (MAX_LINE - 1), 0)
    found_b = prev >= lo
    start = np.where(found_b, prev + 1, lo)
    binary = np.where(found_b, b[np.maximum(prev, 0)] == 0 if L else False, o >= MAX_LINE - 1)
    # forward: the first stop in [o, min(L, o + 1024))
    k = np.searchsorted(stops, o, side="left")
    nxt = np.where(k < len(stops), stops[np.minimum(k, len(stops) - 1)] if len(stops) else L + MAX_LINE, L + MAX_LINE)
    hi = np.minimum(L, o + MAX_LINE)
    found_f = nxt < hi
    ran_out = ~found_f & (L - o >= MAX_LINE)
    end = np.where(found_f, nxt, np.where(ran_out, o + MAX_LINE - 1, np.where(L > o, L - 1, o)))
    binary = binary | np.where(found_f, b[np.minimum(nxt, max(L - 1, 0))] == 0 if L else False, ran_out)
    return start, (end - start).astype(np.int32), binary.astype(bool)


class Lines:
    """every anchor of a fixture: what femto_amd_lines answers for text offsets (arrays over the prepared text's positions)"""

    def __init__(self, fx):
        self.docs = fx.docs
        self.doc_ends = np.cumsum([len(d) + 1 for d in fx.docs]).astype(np.int64)
        self.doc_starts = np.concatenate([[0], self.doc_ends[:-1]]).astype(np.int64)
        self.N = int(self.doc_ends[-1])
        self.text = np.concatenate([np.concatenate([d, np.zeros(1, dtype=np.uint8)]) for d in fx.docs])     # (SEOF slots: 0, never read)
        self.doc = np.zeros(self.N, dtype=np.int64)
        self.pos = np.zeros(self.N, dtype=np.int64)
        self.len = np.zeros(self.N, dtype=np.int32)
        self.binary = np.zeros(self.N, dtype=bool)
        for d, b in enumerate(fx.docs):
            s = int(self.doc_starts[d])
            st, ln, bi = lines_of_document(b, np.arange(len(b) + 1))
            self.doc[s:s + len(b) + 1] = d
            self.pos[s:s + len(b) + 1] = st + s
            self.len[s:s + len(b) + 1] = ln
            self.binary[s:s + len(b) + 1] = bi

    def answer(self, offsets):
        """(doc, pos, len, flags) for any int64 offsets (out of range: -1, -1, 0, INVALID)"""
        p = np.asarray(offsets, dtype=np.int64)
        ok = (p >= 0) & (p < self.N)
        q = np.where(ok, p, 0)
        return (np.where(ok, self.doc[q], -1), np.where(ok, self.pos[q], -1), np.where(ok, self.len[q], 0).astype(np.int32),
                np.where(ok, self.binary[q].astype(np.uint8) * BINARY, INVALID).astype(np.uint8))

    def packed(self, pos, lens):
        """(byte_starts, bytes) of the lines one after another"""
        lens = np.asarray(lens, dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if starts[-1] == 0:
            return starts, np.zeros(0, dtype=np.uint8)
        src = np.repeat(np.asarray(pos, dtype=np.int64) - starts[:-1], lens) + np.arange(starts[-1])
        return starts, self.text[src]

    def line(self, p):
        return bytes(self.text[int(self.pos[p]):int(self.pos[p]) + int(self.len[p])])


def group_first(starts, data, flags=None):
    """(group_first, number of distinct lines): group_first[i] = the least j with the same bytes as line i; -1 where INVALID"""
    n = len(starts) - 1
    seen = {}
    out = np.full(n, -1, dtype=np.int64)
    raw = bytes(np.asarray(data, dtype=np.uint8))
    for i in range(n):
        if flags is not None and flags[i] & INVALID:
            continue
        out[i] = seen.setdefault(raw[int(starts[i]):int(starts[i + 1])], i)
    return out, len(seen)


# ---- the search tool's output (search_tool.cc:227-351, 412-522), formatted here from the restatement --------------------------

def _json_str(s):
    out = []
    for c in s:
        if c == 0x22:
            out.append('\\"')
        elif c == 0x5c:
            out.append("\\\\")
        elif 32 <= c < 127:
            out.append(chr(c))
        else:
            out.append("\\u%04x" % c)
    return "".join(out).encode()


def _json_info(info):
    return b'"' + b'","'.join(_json_str(part) for part in info.split(b"|")) + b'"'


def format_lines(hits, infos, doclens, lines, sep=b"\n", json=False, echo=b""):
    """--lines: hits = [(doc, text position of the anchor)] in (document, offset) order; lines: a Lines"""
    out = []
    first = True
    for d, p in hits:
        binary, line = bool(lines.binary[p]), lines.line(p)
        if json:
            row = b"[ [" + _json_info(infos[d]) + b"]," + (b"[]" if binary else b'"' + _json_str(line) + b'"') + b", %d]" % doclens[d]
            out.append((b"" if first else b",\n   ") + row)
            first = False
        elif binary:
            out.append(infos[d] + (b"\0" if sep == b"\0" else b":") + b" matches" + sep)
        else:
            out.append(infos[d] + (b"\0" if sep == b"\0" else b":") + line + sep)
    return _wrap(out, bool(hits), sep, json, echo)


def format_multilines(hits, infos, doclens, lines, sep=b"\n", json=False, echo=b""):
    """--multilines: one entry per distinct line, lines in strcmp order, each with its documents sorted and de-duplicated"""
    groups = {}
    for d, p in hits:
        groups.setdefault(lines.line(p), set()).add((infos[d], doclens[d]))
    out = []
    first = True
    for line in sorted(groups):
        docs = sorted(groups[line])
        seen, uniq = set(), []
        for info, dl in docs:          # cmpleninfo compares the info strings only
            if info not in seen:
                seen.add(info)
                uniq.append((info, dl))
        if json:
            row = (b"[ [" + b", ".join(_json_info(i) for i, _ in uniq) + b'],"' + _json_str(line) + b'", [' +
                   b", ".join(b",".join([b"%d" % dl] * (1 + i.count(b"|"))) for i, dl in uniq) + b"] ]")
            out.append((b"" if first else b",\n   ") + row)
            first = False
        else:
            out.append(b"|".join(i for i, _ in uniq) + (b"\0" if sep == b"\0" else b":") + line + sep)
    return _wrap(out, bool(hits), sep, json, echo)


def _wrap(rows, any_hit, sep, json, echo):
    body = b"".join(rows)
    if json:
        return b'{\n "pattern":"' + _json_str(echo) + b'",\n "results":[\n   ' + body + b" ]\n}\n"
    return body + (sep if any_hit else b"")
