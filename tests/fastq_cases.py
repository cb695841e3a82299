"""The FASTQ texts the parser tests read (CPU and GPU files share them): (name, text, min_letters), valid ones and ones with
an error.  Their sizes are placed by the library's own: T bytes of text per tile, S tile counts (and chunk sums) per step of
the one-workgroup scans, C records per chunk -- read from the header, so nothing here hard-codes them."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    h = open(os.path.join(ROOT, "include", "abismal_amd.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, h).group(1))


T = _define("ABM_FASTQ_TILE_BYTES")
S = _define("ABM_FASTQ_SCAN_TILES")
C = _define("ABM_FASTQ_CHUNK_RECORDS")
SCAN_LEVELS = [S]   # every size at which a scan changes level: the one-workgroup scans take S values per step
MAX_READ = 32766    # the longest read that is not an error

TILE_COUNTS = [1, 2, 63, 64, 65, S - 1, S, S + 1]
RECORD_COUNTS = [1, 2, 63, 64, 65, C - 1, C, C + 1, 4095, 4096, 4097]


def _bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def rec(name, seq, plus=b"+", qual=None):
    """one record's four lines, each with its newline; name without the leading '@'"""
    return b"@" + name + b"\n" + seq + b"\n" + plus + b"\n" + (b"I" * len(seq) if qual is None else qual) + b"\n"


def mixed(n, seed, trailing_newline=True):
    """n records of lengths 30 ... 151: N at both ends, too few informative bases, Ns inside, names with a description, a
    tab, a slash or nothing after them (the mix of write_fastq in tests/test_cli_fastq_host.py)"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([30, 44, 45, 50, 100, 100, 100, 151], size=n)
    kinds = rng.random(n)
    tails = rng.integers(0, 4, size=n)
    pool = _bases(rng, int(lens.sum()))
    out, at = [], 0
    for i in range(n):
        L = int(lens[i])
        seq = pool[at:at + L]
        at += L
        k = kinds[i]
        if k < 0.15:
            seq = b"N" * (1 + i % 6) + seq + b"N" * (1 + i % 9)
        elif k < 0.25:
            seq = seq[:20] + b"N" * (L - 20)
        elif k < 0.30:
            seq = seq[:10] + b"NN" + seq[12:]
        name = b"read%d" % i + (b"", b" desc 1:N:0", b"\tx", b"/1")[tails[i]]
        out.append(rec(name, seq))
    text = b"".join(out)
    return text if trailing_newline else text[:-1]


def sized(n_bytes, seed):
    """a valid text of exactly n_bytes (at least 400): records of 100 bases, every few of them with a long description in
    its name line, the last one's padded so that the text ends where it should"""
    rng = np.random.default_rng(seed)
    out, have, i = [], 0, 0
    while True:
        seq = _bases(rng, 100)
        name = b"s%d pad " % i
        base = len(rec(name, seq))
        left = n_bytes - have
        if left <= 30000 + base + 400:
            assert left >= base
            out.append(rec(name + b"x" * (left - base), seq))
            break
        pad = int(rng.integers(9000, 30000)) if i % 5 == 2 and left > 100000 else 0
        out.append(rec(name + b"x" * pad, seq))
        have += base + pad
        i += 1
    text = b"".join(out)
    assert len(text) == n_bytes
    return text


def _filler(n_tiles, seed):
    """ordinary records that fill a little more than n_tiles tiles (nothing for 0)"""
    if not n_tiles:
        return b""
    text = mixed(n_tiles * T // 150, seed)
    assert len(text) > n_tiles * T
    return text


def _name_line_ending_at(prefix, pos):
    """prefix + a record whose name line's newline is byte `pos` of the whole text"""
    assert pos >= len(prefix) + 1
    return prefix + rec(b"e" * (pos - len(prefix) - 1), b"ACGT" * 25)


def _tile_edge_cases():
    out = []
    rng = np.random.default_rng(11)
    for where, tiles in (("record 0", 0), ("a later tile", 3)):
        pre = _filler(tiles, 12)
        edge = (len(pre) // T + 1) * T  # the first tile boundary that a name line after `pre` can reach
        if edge - len(pre) < 8:
            edge += T
        out.append(("newline on a tile's last byte, %s" % where, _name_line_ending_at(pre, edge - 1) + mixed(3, 1), 44))
        out.append(("newline on a tile's first byte, %s" % where, _name_line_ending_at(pre, edge) + mixed(3, 2), 44))
        # the sequence line's newline on the edge too (its line begins 3 bytes after the record does)
        for at, what in ((edge - 1, "last"), (edge, "first")):
            seq = _bases(rng, at - len(pre) - 3)
            out.append(("sequence newline on a tile's %s byte, %s" % (what, where), pre + rec(b"q", seq) + mixed(2, 3), 44))
        out.append(("a record over two tiles, %s" % where, pre + rec(b"two", _bases(rng, T)) + mixed(2, 4), 44))
        out.append(("a record over three tiles, %s" % where, pre + rec(b"three x", _bases(rng, 2 * T + 100)) + mixed(2, 5), 44))
        out.append(("a name line of 9000 bytes, %s" % where, pre + rec(b"long " + b"d" * 8994, _bases(rng, 100)) + mixed(2, 6), 44))
        out.append(("a name line of 20000 bytes without a blank, %s" % where, pre + rec(b"L" * 19999, _bases(rng, 100)) + mixed(2, 7), 44))
        out.append(("a name line of 9000 bytes whose blank is its last byte, %s" % where, pre + rec(b"b" * 8998 + b" ", _bases(rng, 60)), 44))
        out.append(("a read of 32766 bases, %s" % where, pre + rec(b"max", _bases(rng, MAX_READ)) + mixed(2, 8), 44))
        out.append(("a read of 32766 bases, Ns at both ends, %s" % where, pre + rec(b"maxN", b"N" * 5000 + _bases(rng, MAX_READ - 9000) + b"N" * 4000), 44))
        out.append(("tiles without any newline, %s" % where, pre + rec(b"q", _bases(rng, 100), qual=b"#" * (3 * T)) + mixed(2, 9), 44))
    return out


def _rule_cases():
    a = b"ACGT" * 11  # 44 letters
    return [
        ("43 informative at 44", rec(b"r", a[:43] + b"NNN"), 44),
        ("44 informative at 44", rec(b"r", a + b"NNN"), 44),
        ("35 informative at 36", rec(b"r", a[:35] + b"N"), 36),
        ("36 informative at 36", rec(b"r", b"N" + a[:36]), 36),
        ("all N", rec(b"r", b"N" * 80), 44),
        ("N at both ends", rec(b"r", b"NNN" + a + a + b"NNNNN"), 44),
        ("N at the head only", rec(b"r", b"NN" + a + a), 44),
        ("N at the tail only", rec(b"r", a + a + b"N"), 44),
        ("N inside", rec(b"r", a + b"NNNN" + a), 44),
        # 44 informative bytes of which the first four are no bases: the read that is left has 40 letters
        ("leading R, Y and lower case trim 44 informative below 44", rec(b"r", b"RYac" + a[:40]), 44),
        ("leading non-bases after leading N", rec(b"r", b"NNRYacgt" + a + b"NN"), 44),
        ("CR LF line ends", b"@r one\r\n" + a + a + b"\r\n+\r\n" + b"I" * 88 + b"\r\n@s\r\n" + a + b"NN\r\n+\r\n\r\n", 44),
        ("a name with a space", rec(b"name rest of it", a), 44),
        ("a name with a tab", rec(b"name\trest", a), 44),
        ("a name with neither", rec(b"name/1", a), 44),
        ("a name with a tab before a space", rec(b"na\tme rest", a), 44),
        ("@ alone", rec(b"", a), 44),
        ("@ and a blank", rec(b" x", a), 44),
        ("a name line that begins with a blank", b" xy z\n" + a + b"\n+\n\n", 44),
        ("empty + and quality lines", rec(b"r", a, plus=b"", qual=b"") + rec(b"s", a, plus=b"", qual=b""), 44),
        ("a quality line that begins with @", rec(b"r", a, qual=b"@" + b"I" * 43) + rec(b"s", a), 44),
        ("a quality line that begins with +", rec(b"r", a, qual=b"+" + b"I" * 43) + rec(b"s", a), 44),
        ("a + line that repeats the name", rec(b"r", a, plus=b"+r") + rec(b"s", a, plus=b"+s"), 44),
        ("an empty sequence line", rec(b"r", b"") + rec(b"s", a), 44),
    ]


def _small_texts():
    a = b"ACGT" * 12
    out = [("empty", b"", 44), ("one byte", b"@", 44), ("one byte, a letter", b"A", 44),
           ("a name line alone", b"@lonely", 44), ("a name line alone with its newline", b"@lonely\n", 44)]
    full = rec(b"r x", a)
    nl = [k for k, c in enumerate(full) if c == 10]
    for what, cut in (("the sequence line", nl[1]), ("the + line", nl[2]), ("the quality line", nl[3])):
        out.append(("ends after %s" % what, full[:cut], 44))
        out.append(("ends after %s and its newline" % what, full[:cut + 1], 44))
        out.append(("two records, ends after %s" % what, full + full[:cut], 44))
    out.append(("records and a trailing name line", full + full + b"@trailing", 44))
    return out


def _error_cases():
    a = b"ACGT" * 12
    rng = np.random.default_rng(13)
    pre = _filler(3, 14)
    n_pre = pre.count(b"\n") // 4
    long_read = _bases(rng, MAX_READ + 1)
    return [
        ("error: a newline alone", b"\n", 44),
        ("error: an empty name line", rec(b"r", a) + b"\n" + a + b"\n+\n\n", 44),
        ("error: an empty trailing name line", rec(b"r", a) + b"\n", 44),
        ("error: a read of 32767 bytes", rec(b"r", a) + rec(b"big", long_read), 44),
        ("error: a read of 40000 bytes of N", rec(b"big", b"N" * 40000) + rec(b"r", a), 44),
        ("error: 50 x R", rec(b"r", a) + rec(b"nobase", b"R" * 50) + rec(b"s", a), 44),
        ("error: lower case only", rec(b"nobase", b"acgt" * 12), 44),
        ("error: empty name in the first tile, too long later", b"\n" + a + b"\n+\n\n" + pre + rec(b"big", long_read), 44),
        ("error: too long in the first tile, empty name later", rec(b"big", long_read) + pre + b"\n" + a + b"\n+\n\n", 44),
        ("error: no base first, too long later", rec(b"nobase", b"Y" * 60) + pre + rec(b"big", long_read) + mixed(2, 1), 44),
        ("error: too long first, no base later", pre + rec(b"big", long_read) + pre + rec(b"nobase", b"Y" * 60), 44),
        ("error: in the text's last record", pre + rec(b"nobase", b"R" * 50), 44),
        ("error: in the text's last record, no final newline", pre + rec(b"nobase", b"R" * 50)[:-1], 44),
        ("error: a too long last line without a newline", pre + b"@big\n" + long_read, 44),
        ("error: no base at 36 letters", rec(b"nobase", b"K" * 36), 36),
        ("error: many, the first at record %d" % n_pre, pre + b"".join(rec(b"nobase", b"R" * 50) for _ in range(3 * C)), 44),
    ]


BIG = "mixed, 70000 records"


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, text, min_letters)]"""
    out = _small_texts() + _rule_cases() + _tile_edge_cases()
    for k in TILE_COUNTS:
        out.append(("%d tiles" % k, sized(k * T - 17, k), 44))
    for k in (1, 2, 64, S):
        out.append(("%d tiles to their last byte" % k, sized(k * T, 100 + k), 44))
        out.append(("%d tiles and one byte" % k, sized(k * T + 1, 200 + k), 44))
    for n in RECORD_COUNTS:
        out.append(("%d records" % n, mixed(n, 300 + n, trailing_newline=n % 2 == 0), 44 if n % 3 else 36))
    # more chunks than one step of the chunk scan takes: S * C + 1 records of seven bytes, all cut to empty
    out.append(("%d records of seven bytes" % (S * C + 1), b"@\nA\n+\n\n" * (S * C) + b"@\nA", 44))
    out.append((BIG, mixed(70000, 7), 44))
    out += _error_cases()
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def by_name(name):
    return next(c for c in cases() if c[0] == name)


def is_error(name):
    return name.startswith("error:")
