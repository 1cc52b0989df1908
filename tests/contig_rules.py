"""The name rule of DNA_ExtractChrPileupData (dna_sv_tensor/src/extract_chr_pileup_data/main.cpp:11-80), restated in Python: test
infrastructure shared by the CPU test that pins it against the reference's own output (tests/golden/extract_chr.npz) and the GPU tests
whose expectations rest on it."""
import numpy as np

KEY_SHIFT = 36
FILLER = -(1 << 62)
SPACE = b" \t\n\v\f\r"                                    # isspace of the C locale


def line_spans(text):
    """[(start, end)] of the reader's lines: a '\\n' or the end of the text ends a line (line_reader.cpp:95-127)"""
    spans, s = [], 0
    while s < len(text):
        e = text.find(b"\n", s)
        e = len(text) if e < 0 else e
        spans.append((s, e))
        s = e + 1
    return spans


def line_name(line):
    """extract_char_name: the bytes in front of the first isspace byte"""
    n = 0
    while n < len(line) and line[n] not in SPACE:
        n += 1
    return line[:n]


def contig_rule(text, names, seqs, pos):
    """text: bytes; names: the table's names (bytes) with their sequences seqs (uint8 arrays); pos: the position of every line ->
    (cid int32 [M], ref uint8 [M], key int64 [M], runs int64 [R, 2]): a name is looked up only where it differs from the line in front"""
    cid, ref, key, runs, last, c = [], [], [], [], None, -1
    for i, (s, e) in enumerate(line_spans(text)):
        name = line_name(text[s:e])
        if i == 0 or name != last:
            c = names.index(name) if name in names else -1
            runs.append((i, c)); last = name
        cid.append(c)
        known = c >= 0 and 1 <= pos[i] <= len(seqs[c])
        ref.append(seqs[c][pos[i] - 1] if known else ord("N"))
        key.append((c << KEY_SHIFT) | int(pos[i]) if known else FILLER)
    return np.array(cid, np.int32), np.array(ref, np.uint8), np.array(key, np.int64), np.array(runs, np.int64).reshape(-1, 2)


def split_by_contig(text, wanted):
    """what the splitter leaves in its output directory: {name: bytes of <name>.mpileup}.  Empty lines are skipped, one '\\r' in front of
    the '\\n' is dropped, a name that comes again re-opens its file with "w" """
    files, last, out = {}, b"", None
    for s, e in line_spans(text):
        line = text[s:e - 1] if e > s and e < len(text) and text[e - 1:e] == b"\r" else text[s:e]
        if not line:
            continue
        name = line_name(line)
        if name != last:
            last = name
            out = name if name in wanted else None
            if out is not None:
                files[out] = b""
        if out is not None:
            files[out] += line + b"\n"
    return files
