"""Plain-Python restatement of the BAM records of `abismal-amd map -B` (put_bam_record of abm_cli_records.hpp) in the two parts
the kernels and the host make them from (include/abismal_amd.h): piece() builds a record without its name from the
fields tests/sam_format.py's record() takes, assemble() puts the name in by the host's four steps."""
import struct

NT16 = "=ACMGRSVTWYHKDBN"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
_OPS = "MIDNSHP=XB"


def reg2bin(beg, end):
    end -= 1
    for shift, level in ((14, 15), (17, 12), (20, 9), (23, 6), (26, 3)):
        if beg >> shift == end >> shift:
            return ((1 << level) - 1) // 7 + (beg >> shift)
    return 0


def ref_len(cig):
    return sum(int(v) >> 4 for v in cig if (int(v) & 15) in (0, 2, 3, 7, 8))


def seq_codes(seq, rc):
    """the 4-bit codes of what SEQ shows (sam_format.seq_text, then the letter's index in NT16)"""
    if rc:
        shown = [_COMP.get(c, "N") for c in reversed(seq)]
    else:
        shown = []
        for c in seq:
            u = c.upper() if "a" <= c <= "z" else c
            shown.append(u if u in NT16 else "N")
    return [NT16.index(c) for c in shown]


def piece(flag, refid, pos, cig, rnext, pnext, tlen, seq, rc, nm, cv):
    """record() of sam_format with the chromosome's number in the BAM header in the place of its name: pos 0-based,
    rnext "=" (the mate on the same chromosome, pnext its 1-based POS) or "*" (none)"""
    cig = [int(v) for v in cig]
    rl = ref_len(cig)
    next_refid = refid if rnext == "=" else -1
    next_pos = pnext - 1 if rnext == "=" else -1
    codes = seq_codes(seq, rc)
    packed = bytearray()
    for i in range(0, len(codes), 2):
        packed.append(codes[i] << 4 | (codes[i + 1] if i + 1 < len(codes) else 0))
    if 0 <= nm <= 255:
        tag = b"NMC" + struct.pack("<B", nm)
    elif nm >= 0:
        tag = b"NMS" + struct.pack("<H", nm)
    elif nm >= -128:
        tag = b"NMc" + struct.pack("<b", nm)
    else:
        tag = b"NMs" + struct.pack("<h", nm)
    body = (struct.pack("<iIBBHHHIiii", refid, pos, 0, 255, reg2bin(pos, pos + (rl if rl else 1)) & 0xFFFF, len(cig), flag,
                        len(codes), next_refid, next_pos, tlen)
            + b"".join(struct.pack("<I", v) for v in cig) + bytes(packed) + b"\xff" * len(codes) + tag + b"CVA" + cv.encode())
    return struct.pack("<I", len(body)) + body


def assemble(name, pc):
    """the host's four steps: the 36 fixed bytes, block_size and l_read_name taking the name in, the name and a NUL, the rest"""
    if isinstance(name, str):
        name = name.encode()
    head = bytearray(pc[:36])
    struct.pack_into("<I", head, 0, struct.unpack_from("<I", head, 0)[0] + len(name) + 1)
    head[12] = (len(name) + 1) & 0xFF
    return bytes(head) + name + b"\0" + pc[36:]


def parse_cigar(text):
    out, n = [], 0
    for c in text:
        if c.isdigit():
            n = n * 10 + int(c)
        else:
            out.append(n << 4 | _OPS.index(c))
            n = 0
    return out


def piece_from_tail(tail, refids):
    """the piece of a SAM record after QNAME (sam_format.record's bytes; refids: chromosome name -> number in the header);
    b"" stays b"".  SEQ is already what the record shows, so its letters are coded as they stand."""
    if not tail:
        return b""
    f = tail.decode().rstrip("\n").split("\t")
    assert f[0] == "" and f[4] == "255" and f[10] == "*" and f[11].startswith("NM:i:") and f[12].startswith("CV:A:"), tail
    return piece(int(f[1]), refids[f[2]], int(f[3]) - 1, parse_cigar(f[5]), f[6], int(f[7]), int(f[8]), f[9], False,
                 int(f[11][5:]), f[12][5:])


def records_of_stream(raw):
    """the alignment records of a decompressed BAM stream, each with its block_size: (header bytes, [records])"""
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, at)
    at += 4
    names = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", raw, at)
        names.append(raw[at + 4:at + 4 + l_name - 1].decode())
        at += 4 + l_name + 4
    header, recs = raw[:at], []
    while at < len(raw):
        bs, = struct.unpack_from("<I", raw, at)
        recs.append(raw[at:at + 4 + bs])
        at += 4 + bs
    return header, names, recs


def bgzf_decompress(data):
    import zlib
    out, at = [], 0
    while at < len(data):
        d = zlib.decompressobj(31)
        out.append(d.decompress(data[at:]))
        assert d.eof
        at = len(data) - len(d.unused_data)
    return b"".join(out)
