"""Plain-Python restatement of the CLI's paired-end SAM formatting (emit_pe / emit_se / put_record of abm_cli_records.hpp,
after select_output and format_pe / format_se of the reference) over map_pe's returned arrays and the index's
chromosome table: each end's record without QNAME, as the pair kernels write it (abm_ctx_pe_sam_tails)."""
import bisect

_IUPAC = set("=ABCDGHKMNRSTVWY")
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def ref_len(cig):
    return sum(int(v) >> 4 for v in cig if (int(v) & 15) in (0, 2, 3, 7, 8))


def locate(starts, pos, reflen):
    """Chroms::locate: (chromosome index, 0-based offset) or None"""
    k = bisect.bisect_right(starts, pos)
    if k == 0:
        return None
    c = k - 1
    if c + 1 >= len(starts) or pos + reflen > starts[c + 1]:
        return None
    return c, pos - starts[c]


def seq_text(seq, rc):
    if rc:
        return "".join(_COMP.get(c, "N") for c in reversed(seq))
    out = []
    for c in seq:
        u = c.upper() if "a" <= c <= "z" else c
        out.append(u if u in _IUPAC else "N")
    return "".join(out)


def cigar_text(cig):
    return "".join(f"{int(v) >> 4}{'MIDNSHP=XB'[min(int(v) & 15, 9)]}" for v in cig)


def record(flag, rname, pos, cig, rnext, pnext, tlen, seq, rc, nm, cv):
    return (f"\t{flag}\t{rname}\t{pos + 1}\t255\t{cigar_text(cig)}\t{rnext}\t{pnext}\t{tlen}\t{seq_text(seq, rc)}"
            f"\t*\tNM:i:{nm}\tCV:A:{cv}\n").encode()


def format_pair(allow_ambig, names, starts, pair, h1, h2, s1, s2, c1, c2):
    """select_output for one pair: (kind, tail of end 1, tail of end 2) with kind 0 = the pair's records, 1 = single-end
    records (b"" = no record for that end)"""
    p1, p2 = pair["r1"], pair["r2"]
    if int(p1["pos"]) != 0 and (allow_ambig or not int(p1["flags"]) & 0x100):
        l1, l2 = locate(starts, int(p1["pos"]), ref_len(c1)), locate(starts, int(p2["pos"]), ref_len(c2))
        if l1 and l2 and l1[0] == l2[0]:
            (ch, b1), (_, b2) = l1, l2
            e2 = b2 + ref_len(c2)
            rc1, rc2 = bool(int(p1["flags"]) & 0x10), bool(int(p2["flags"]) & 0x10)
            isize = b1 - e2 if rc1 else e2 - b1
            f1, f2 = 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80
            if rc1:
                f1 |= 0x10
                f2 |= 0x20
            if rc2:
                f2 |= 0x10
                f1 |= 0x20
            if allow_ambig and int(p1["flags"]) & 0x100:
                f1 |= 0x100
                f2 |= 0x100
            cv1 = "A" if int(p1["flags"]) & 0x1000 else "T"
            cv2 = "A" if int(p2["flags"]) & 0x1000 else "T"
            return (0, record(f1, names[ch], b1, c1, "=", b2 + 1, isize, s1, rc1, int(p1["diffs"]), cv1),
                    record(f2, names[ch], b2, c2, "=", b1 + 1, -isize, s2, rc2, int(p2["diffs"]), cv2))
    tails = []
    for h, s, c in ((h1, s1, c1), (h2, s2, c2)):
        amb = bool(int(h["flags"]) & 0x100)
        loc = locate(starts, int(h["pos"]), ref_len(c)) if int(h["pos"]) != 0 and (allow_ambig or not amb) else None
        if loc is None:
            tails.append(b"")
            continue
        rc = bool(int(h["flags"]) & 0x10)
        flag = (0x10 if rc else 0) | (0x100 if allow_ambig and amb else 0)
        tails.append(record(flag, names[loc[0]], loc[1], c, "*", 0, 0, s, rc, int(h["diffs"]),
                            "A" if int(h["flags"]) & 0x1000 else "T"))
    return (1, tails[0], tails[1])


def format_batch(allow_ambig, index, reads1, reads2, result):
    """format_pair over a map_pe result (pairs, se1, se2, (cig1, off1), (cig2, off2), ...) for every pair"""
    pairs, se1, se2, (c1, o1), (c2, o2) = result[:5]
    names = list(index.chrom_names)
    starts = [int(x) for x in index.chrom_starts[:len(names) + 1]]
    out = []
    for i in range(len(pairs)):
        out.append(format_pair(allow_ambig, names, starts, pairs[i], se1[i], se2[i], reads1[i], reads2[i],
                               c1[int(o1[i]):int(o1[i + 1])], c2[int(o2[i]):int(o2[i + 1])]))
    return out
