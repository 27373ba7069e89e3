"""Plain-Python restatement of ma_select_records_batch (include/microasm.h): the candidates of every window in, the record bits,
the window states, the per-sample sums and the selected lists out.  Parses the record bytes with flatten_ref.parse_record,
walks the auxiliary fields and the MD string byte by byte, keeps the events in Counters.  Imports neither the engine nor the
host shell: tests hold both to it."""
import struct
from collections import Counter

import numpy as np

from flatten_ref import parse_record

MA_SK_COLLECT, MA_SK_ELIGIBLE = 1, 2
MA_S_ACTIVE, MA_S_LOW_COVERAGE, MA_S_CAPPED, MA_S_MD_RANGE, MA_S_EVENTS, MA_S_LISTED = 1, 2, 4, 8, 16, 32
MA_S_HOST_BITS = MA_S_CAPPED | MA_S_MD_RANGE | MA_S_EVENTS
MA_ERR_ARG = -1
EVENT_KEYS = 8192
MISMATCH, INSERTION, DELETION, SOFTCLIP = range(4)
U32 = 0xFFFFFFFF
TAG_BYTES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


class SelectError(Exception):
    def __init__(self, rc, what, record=None):
        super().__init__(what)
        self.rc, self.record = rc, record


def core_bytes(b):
    """bytes of a good record up to the end of its qualities"""
    l_name, n_cigar, l_seq = b[8], struct.unpack_from("<H", b, 12)[0], struct.unpack_from("<i", b, 16)[0]
    return 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq


def find_md(b):
    """the last MD:Z of the auxiliary fields of record bytes `b` (cut where the caller cut them), or None"""
    p, end, md = core_bytes(b), len(b), None
    while p + 3 <= end:
        tag, ty = b[p:p + 2], chr(b[p + 2])
        p += 3
        if ty in "ZH":
            nul = b.find(b"\0", p)
            if nul < 0:
                break
            if tag == b"MD" and ty == "Z":
                md = b[p:nul]
            size = nul - p + 1
        elif ty in TAG_BYTES:
            size = TAG_BYTES[ty]
        elif ty == "B":
            if p + 5 > end:
                break
            count = struct.unpack_from("<i", b, p + 1)[0]
            if count < 0:
                break
            size = 5 + count * {"c": 1, "C": 1, "s": 2, "S": 2}.get(chr(b[p]), 4)
        else:
            break
        if size > end - p:
            break
        p += size
    return md


def record_events(r, md):
    """-> (list of (multiset, position), the MD walk left the read)"""
    events, out_of_range = [], False
    start = r["pos"] & U32
    if r["pos"] >= 0 and md is not None:
        gpos, digits = start, b""
        for ch in md:
            if 0x30 <= ch <= 0x39:
                digits += bytes([ch])
                continue
            if len(digits) > 9:
                out_of_range = True
                break
            gpos = (gpos + (int(digits) if digits else 0)) & U32
            digits = b""
            at = (gpos - start) & U32
            if at >= r["l_seq"]:
                out_of_range = True
                break
            if r["qual"][at] < 20:
                continue
            if bytes([ch]).upper() in (b"A", b"C", b"G", b"T"):
                events.append((MISMATCH, gpos))
    gpos = start
    for ln, op in r["cigar"]:
        if op in (0, 2, 3, 7, 8):
            gpos = (gpos + ln) & U32
        if op == 1:
            events.append((INSERTION, gpos))
        elif op == 2:
            events.append((DELETION, gpos))
        elif op == 8:
            events.append((MISMATCH, gpos))
        elif op == 4:
            events.append((SOFTCLIP, gpos))
    return events, out_of_range


def record_bits(r):
    usable = not r["flag"] & (0x200 | 0x400 | 0x4)
    return (MA_SK_COLLECT if usable and r["mapq"] >= 20 else 0) | (MA_SK_ELIGIBLE if usable and r["mapq"] != 0 else 0)


def select(rec, n_windows, n_records, n_samples, win_len, max_sample_cov=1000.0, min_anchor_cov=5, skip_active_region=False,
           event_keys=EVENT_KEYS):
    """rec: dict with blob, rec_off, rec_len, rec_win_off, rec_sample.  Returns a dict of the ma_select_out_t arrays, the four
    sel_ arrays n_selected long.  Raises SelectError."""
    blob = np.asarray(rec["blob"], dtype=np.uint8).tobytes()
    rec_off = [int(x) for x in np.asarray(rec["rec_off"])[:n_records]]
    rec_len = [int(x) for x in np.asarray(rec["rec_len"])[:n_records]]
    win_off = [int(x) for x in np.asarray(rec["rec_win_off"])[:n_windows + 1]]
    smp = [int(x) for x in np.asarray(rec["rec_sample"])[:n_records]]
    if win_off[0] != 0 or win_off[-1] != n_records or any(b < a for a, b in zip(win_off, win_off[1:])):
        raise SelectError(MA_ERR_ARG, "rec_win_off does not rise from 0 to n_records")
    parsed = []
    for i in range(n_records):
        r = parse_record(blob, rec_off[i], rec_len[i]) if smp[i] < n_samples else None
        if r is None:
            raise SelectError(MA_ERR_ARG, "record %d is bad" % i, record=i)
        parsed.append(r)
    out = dict(rec_keep=np.zeros(n_records, np.uint8), win_state=np.zeros(n_windows, np.uint8),
               win_sample_reads=np.zeros(n_windows * n_samples, np.uint32), win_sample_bases=np.zeros(n_windows * n_samples, np.uint64),
               n_selected=np.zeros(1, np.uint64), sel_win_off=np.zeros(n_windows + 1, np.uint32),
               either=np.zeros(n_windows, bool))  # (not an output of the call: windows that may be MA_S_EVENTS instead of active)
    sel = []
    for w in range(n_windows):
        members = range(win_off[w], win_off[w + 1])
        reads, bases = [0] * n_samples, [0] * n_samples
        counts = [Counter() for _ in range(n_samples)]
        md_range = False
        for i in members:
            bits = record_bits(parsed[i])
            out["rec_keep"][i] = bits
            if bits & MA_SK_COLLECT:
                reads[smp[i]] += 1
                bases[smp[i]] += parsed[i]["l_seq"]
            if bits & MA_SK_ELIGIBLE and not skip_active_region:
                events, bad = record_events(parsed[i], find_md(blob[rec_off[i]:rec_off[i] + rec_len[i]]))
                counts[smp[i]].update(events)
                md_range = md_range or bad
        state = 0
        if skip_active_region:
            state |= MA_S_ACTIVE
        else:
            if any(c >= 2 for cs in counts for c in cs.values()):
                state |= MA_S_ACTIVE
                # every sample that holds a position twice also holds more keys than the table: the header leaves the call free
                # to report MA_S_EVENTS instead (what it met first).  This restatement answers MA_S_ACTIVE and says so here
                out["either"][w] = all(len(cs) > event_keys for cs in counts if any(c >= 2 for c in cs.values()))
            elif any(len(cs) > event_keys for cs in counts):
                state |= MA_S_EVENTS
            if md_range:
                state |= MA_S_MD_RANGE
        length = np.float64(int(win_len[w]))
        for s in range(n_samples):
            out["win_sample_reads"][w * n_samples + s] = reads[s]
            out["win_sample_bases"][w * n_samples + s] = bases[s]
            if reads[s]:
                with np.errstate(all="ignore"):
                    per_read = np.float64(bases[s]) / np.float64(reads[s])
                    max_reads = np.ceil(np.float64(max_sample_cov) * length / per_read)
                if np.float64(reads[s]) > max_reads:
                    state |= MA_S_CAPPED
        with np.errstate(all="ignore"):
            if np.float64(sum(bases)) / length < np.float64(min_anchor_cov):
                state |= MA_S_LOW_COVERAGE
        if state & MA_S_ACTIVE and not state & (MA_S_HOST_BITS | MA_S_LOW_COVERAGE):
            state |= MA_S_LISTED
            sel += [i for i in members if out["rec_keep"][i] & MA_SK_COLLECT]
        out["win_state"][w] = state
        out["sel_win_off"][w + 1] = len(sel)
    out["n_selected"][0] = len(sel)
    out["sel_src"] = np.array(sel, dtype=np.uint32)
    out["sel_off"] = np.array([rec_off[i] for i in sel], dtype=np.uint64)
    out["sel_len"] = np.array([rec_len[i] for i in sel], dtype=np.uint32)
    out["sel_sample"] = np.array([smp[i] for i in sel], dtype=np.uint8)
    return out


def host_answer(parsed_events):
    """IsActiveRegion's own control flow over one sample's records in order: `parsed_events` is a list of per-record event
    lists in the order CheckAlignment meets them (MD, then I/D/X, then S).  Early returns and all -- the set definition above
    must give the same answer for every order."""
    maps = [Counter() for _ in range(4)]
    for events in parsed_events:
        clipped = False
        for kind, pos in events:
            maps[kind][pos] += 1
            if maps[kind][pos] == 2:
                if kind != SOFTCLIP:
                    return True
                clipped = True  # (the soft-clip loop finishes the record first)
        if clipped:
            return True
    return False

