"""ctypes loader of ``libnanosnp_hip.so`` -- the C ABI declared in include/nanosnp.h.

There is no CPU fallback: importing works everywhere (so the symbol table can be checked on a
machine without a GPU), but creating a :class:`Context` requires the built library and a
gfx950 device and fails loudly otherwise.
"""
from __future__ import annotations

import ctypes as C
import operator
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product always loads the in-tree build.  A/B builds of the same library (tools/build_variant.sh) are loaded only when BOTH
# NANOSNP_DEV_LIB_OVERRIDE=1 and NANOSNP_HIP_LIB=<path> are set: an environment variable alone cannot point the package at an
# arbitrary shared object, and the override says so on stderr.
_OVERRIDE = os.environ.get("NANOSNP_HIP_LIB") if os.environ.get("NANOSNP_DEV_LIB_OVERRIDE") == "1" else None
LIB_PATH = _OVERRIDE or os.path.join(_HERE, "libnanosnp_hip.so")


class NanoSNPError(RuntimeError):
    pass


_SIGNATURES = {
    # name: (restype, argtypes)
    "nsnp_version": (C.c_int, []),
    "nsnp_strerror": (C.c_char_p, [C.c_int]),
    "nsnp_last_hip_error": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p)]),
    "nsnp_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "nsnp_ctx_destroy": (C.c_int, [C.c_void_p]),
    "nsnp_ctx_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "nsnp_ctx_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "nsnp_ctx_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "nsnp_ctx_read_timing": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "nsnp_ctx_shader_clock": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
    "nsnp_pileup_load_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]),
    "nsnp_pileup_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_forward_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_forward_windows_calls": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7),
    "nsnp_pileup_rows_unpack": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 7),
    "nsnp_pileup_postprocess": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "nsnp_pileup_encode_columns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "nsnp_pileup_encode_columns2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    "nsnp_pileup_encode_columns3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                              C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "nsnp_pileup_filter_columns": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 6),
    "nsnp_pileup_filter_columns_keys": (C.c_int, [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 3 + [C.c_int64] * 3 + [C.c_void_p] * 7),
    "nsnp_pileup_encode_columns_keys": (C.c_int, [C.c_void_p] * 5 + [C.c_int64, C.c_double, C.c_double, C.c_int] + [C.c_void_p] * 3 + [C.c_int64] +
                                        [C.c_void_p] * 5),
    "nsnp_pileup_select_sites_range_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_void_p]),
    "nsnp_pileup_select_sites": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_gather_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p]),
    "nsnp_pileup_select_sites_range": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_void_p]),
    "nsnp_pileup_call_rows": (C.c_int, [C.c_void_p] * 8 + [C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_window_records": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "nsnp_pileup_window_records2": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "nsnp_mpileup_line_names": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p]),
    "nsnp_pileup_alt_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_window_records_keys": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                  C.c_int64] + [C.c_void_p] * 5),
    "nsnp_mpileup_line_names_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                                  C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_alt_info_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_label_sites_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "nsnp_pileup_load_indel_heads": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]),
    "nsnp_pileup_label_classes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_forward_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_eval_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "nsnp_pileup_forward_logits2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_eval_windows2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 5),
    "nsnp_pileup_batch_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_train_reserve": (C.c_int, [C.c_void_p, C.c_int64]),
    "nsnp_hap_train_reserve": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int]),
    "nsnp_hap_loss_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_loss_grad": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_float,
                                        C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_optim_scratch_floats": (C.c_int64, [C.c_int, C.c_void_p]),
    "nsnp_optim_step": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 10),
    "nsnp_optim_step_kind": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 12),
    "nsnp_mpileup_tokenise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 6),
    "nsnp_mpileup_tokenise_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int64] * 5 + [C.c_void_p] * 9),
    "nsnp_hap_features": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nsnp_hap_features_i8": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "nsnp_hap_arrange_reads": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "nsnp_hap_arrange_reads2": (C.c_int, [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "nsnp_hap_read_scratch_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "nsnp_hap_read_depths": (C.c_int, [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
    "nsnp_hap_read_matrices": (C.c_int, [C.c_void_p] * 9 + [C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4 +
                               [C.c_int64] + [C.c_void_p] * 4),
    "nsnp_pileup_groups_scratch_bytes": (C.c_size_t, [C.c_int64]),
    "nsnp_pileup_select_groups": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_int] +
                                  [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3),
    "nsnp_hap_load_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int] + [C.c_int] * 5),
    "nsnp_hap_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "nsnp_hap_label_classes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nsnp_hap_train_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "nsnp_pileup_balance_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "nsnp_hap_eval": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "nsnp_hap_batch_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_cat_load_weights": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int]),
    "nsnp_cat_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "nsnp_pileup_forward_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "nsnp_cat_forward_stage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "nsnp_comm_unique_id": (C.c_int, [C.c_void_p]),
    "nsnp_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "nsnp_comm_attach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "nsnp_comm_destroy": (C.c_int, [C.c_void_p]),
    "nsnp_gather_check": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int]),
    "nsnp_gather_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "nsnp_cat_groups": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int] +
                        [C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
}

EXPORTS = tuple(_SIGNATURES)


def tokenise_status_check(status, what="mpileup text"):
    """status word of nsnp_mpileup_tokenise -> ValueError for text the reference's reader aborts on"""
    if status & 1:
        raise ValueError(f"{what}: a line with fewer than five tab-separated fields")
    if status & 2:
        raise ValueError(f"{what}: an empty line")
    if status & 4:
        raise ValueError(f"{what}: position outside the reference sequence")
    if status & 8:
        raise NanoSNPError(f"{what}: tokeniser output buffers too small")
    if status & 16:
        raise ValueError(f"{what}: a contig name longer than {NAME_MAX} bytes")


# nsnp_mpileup_tokenise_contigs (include/nanosnp.h): key = (contig index << KEY_SHIFT) | position, exact in a float64
KEY_SHIFT, MAX_CONTIGS, NAME_MAX = 36, 1 << 17, 255
KEY_FILLER = -(1 << 62)


def check_key_limits(n_contigs, genome_len):
    """the limits a contig table must keep so that every key is exact in a float64 and no step between two contigs is + 1"""
    if n_contigs > MAX_CONTIGS:
        raise NanoSNPError(f"contig table: {n_contigs} contigs, at most {MAX_CONTIGS} share a call")
    if genome_len >= 1 << KEY_SHIFT:
        raise NanoSNPError(f"contig table: {genome_len} bases in all, fewer than 2^{KEY_SHIFT} share a call")


class ContigTable:
    """The wanted contigs of a whole-genome text, resident on the device for Context.mpileup_tokenise_contigs: names_blob + name_off, genome
    (the sequences as stored in the FASTA, back to back) + seq_off; on the host the names and lengths.  contigs: {name: uint8 sequence}
    (in table order), or fasta= a path with names= the wanted names (host.fasta_load_contig reads each)."""

    def __init__(self, contigs=None, fasta=None, names=None, device=0):
        import numpy as np
        import torch
        from . import host
        if contigs is None:
            names = [str(n) for n in names]
            load = lambda n: host.fasta_load_contig(fasta, n)
        else:
            names = [str(n) for n in contigs]
            load = lambda n: np.ascontiguousarray(contigs[n], np.uint8).reshape(-1)
        if len(set(names)) != len(names):
            raise NanoSNPError("contig table: a name is listed twice")
        check_key_limits(len(names), 0)
        if not torch.cuda.is_available():
            raise NanoSNPError("no GPU visible: a contig table lives on the device (nanosnp_amd has no CPU fallback)")
        dev = torch.device("cuda", int(device))
        self.names = names
        # one contig on the host at a time: read, appended to the device genome, dropped (a human genome is 3.1 GB; the device array
        # grows by doubling - copied on the device a few times, cut to size at the end - and is never held on the host as a whole)
        self.lengths, genome, used = [], torch.empty(1 << 20, dtype=torch.uint8, device=dev), 0
        for n in names:
            seq = load(n)
            m = int(seq.size)
            if used + m > genome.numel():
                check_key_limits(len(names), used + m)
                grown = torch.empty(max(used + m, 2 * genome.numel()), dtype=torch.uint8, device=dev)
                grown[:used] = genome[:used]
                genome = grown
            if m:
                genome[used:used + m] = torch.from_numpy(np.array(seq, np.uint8)).to(dev)      # (a copy: the source may be read-only)
            self.lengths.append(m); used += m
            del seq
        self.genome_len = used
        check_key_limits(len(names), used)
        self.genome = genome[:max(used, 1)] if genome.numel() <= used + used // 8 + (1 << 20) else genome[:max(used, 1)].clone()
        del genome                                         # (what the doubling left over goes back to the pool)
        enc = [n.encode() for n in names]
        self.name_off_host = np.concatenate([[0], np.cumsum([len(e) for e in enc])]).astype(np.int64)
        self.seq_off_host = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        up = lambda a, dt: torch.from_numpy(np.array(a, dt)).to(dev)
        self.names_blob = up(np.frombuffer(b"".join(enc) or b"\0", np.uint8), np.uint8)
        self.name_off = up(self.name_off_host, np.int64)
        self.seq_off = up(self.seq_off_host, np.int64)

    def __len__(self):
        return len(self.names)



class BedTable:
    """The BED bitmaps of a whole-genome call beside its ContigTable (include/nanosnp.h, "the bitmap TABLE"): per BED a pair (words: device
    int32 tensor of 32-bit words, off: device int64 [n + 1] word offsets), `ext` for -extended_confident_bed and `conf` for -confident_bed, None
    where there is no such BED.  bed arguments: a path or {contig: intervals} (bed.table_bitmaps says how they are read).  The words travel
    contig by contig through one pinned buffer: a human genome's bitmap is 390 MB per BED and never exists as one host array, as the
    ContigTable never holds the genome on the host."""
    PIN_WORDS = 1 << 22

    def __init__(self, table, extended_bed=None, confident_bed=None, fai=None):
        self.table = table
        self.ext = None if extended_bed is None else self._build(table, extended_bed, fai)
        self.conf = None if confident_bed is None else self._build(table, confident_bed, fai)

    @staticmethod
    def _build(table, bed, fai):
        import numpy as np
        import torch
        from . import bed as _bed
        dev = table.seq_off.device
        iv = _bed.table_intervals(bed, table.names, table.lengths, fai)
        off = _bed.table_word_offsets(iv, table.lengths)
        words = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=dev)[:int(off[-1])]
        pin = torch.empty(BedTable.PIN_WORDS, dtype=torch.int32, pin_memory=True)
        for c, ivc in enumerate(iv):
            if off[c + 1] == off[c]:
                continue
            w = _bed.bed_bitmap(ivc, table.lengths[c]).view(np.int32)
            for a in range(0, w.size, pin.numel()):
                n = min(pin.numel(), w.size - a)
                pin.numpy()[:n] = w[a:a + n]
                words[int(off[c]) + a:int(off[c]) + a + n].copy_(pin[:n], non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()         # (the pinned buffer is written again)
            del w
        return words, torch.from_numpy(off).to(dev)

    @staticmethod
    def upload(table, words, off):
        """host arrays as bed.table_bitmaps returns them -> the device pair (words, off); NanoSNPError unless off is int64 [n + 1], ascending
        from 0 to the number of words"""
        import numpy as np
        import torch
        words = np.ascontiguousarray(words, np.uint32).reshape(-1)
        off = np.ascontiguousarray(off, np.int64).reshape(-1)
        if off.size != len(table) + 1 or off[0] != 0 or bool((np.diff(off) < 0).any()) or int(off[-1]) != words.size:
            raise NanoSNPError("bed table: off must be int64 [n_contigs + 1], ascending from 0 to the number of words")
        dev = table.seq_off.device
        d = torch.empty(max(words.size, 1), dtype=torch.int32, device=dev)[:words.size]
        if words.size:
            d.copy_(torch.from_numpy(words.view(np.int32)))
        return d, torch.from_numpy(off).to(dev)


def _check_bed_pair(bed, table, what):
    import torch
    words, off = bed
    if (words.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not words.is_cuda or not words.is_contiguous()
            or off.dtype != torch.int64 or not off.is_cuda or not off.is_contiguous() or off.numel() != len(table) + 1):
        raise NanoSNPError(f"{what}: bed = (device 32-bit words, device int64 [n_contigs + 1] word offsets) of this contig table (BedTable)")
    return words, off


_lib = None


def load():
    """Loads the shared library (no GPU needed for this) and binds every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NanoSNPError(
            f"{LIB_PATH} not found. The HIP extension is required (there is no CPU fallback): "
            "build it with `make -C nanosnp_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`.")
    # PyTorch-ROCm wheels bundle their own libamdhip64 (soname libamdhip64.so.7).  It has to be the
    # HIP runtime of this process, so it is loaded first; libnanosnp_hip.so's NEEDED entry then
    # resolves to it by soname.  Loading /opt/rocm's copy first would leave two HIP runtimes in one
    # process and every call from the second one fails.
    import torch  # noqa: F401
    if _OVERRIDE:
        import sys
        print(f"nanosnp_amd: DEVELOPMENT OVERRIDE - loading {LIB_PATH} instead of the in-tree library", file=sys.stderr)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, ctx=None, what=""):
    if rc == 0:
        return
    lib = load()
    msg = lib.nsnp_strerror(rc).decode()
    if rc == -3:
        txt = C.c_char_p()
        code = lib.nsnp_last_hip_error(ctx, C.byref(txt))
        msg += f" (hipError {code}: {txt.value.decode() if txt.value else '?'})"
    raise NanoSNPError(f"{what or 'nanosnp'} failed: {msg}")


def _stream_ptr(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class OptimArgs(C.Structure):
    """nsnp_optim_args of include/nanosnp.h: the scalars of one optimiser step, float64 as the caller computed them"""
    _fields_ = [(k, C.c_double) for k in ("max_norm", "weight_decay", "decay", "beta1", "beta2", "eps", "a", "b", "alpha")] + \
               [(k, C.c_int) for k in ("wd_mode", "form", "sync")]


class OptimKindArgs(C.Structure):
    """nsnp_optim_kind_args of include/nanosnp.h: the scalars of one Novograd / SGD / Adadelta step (nsnp_optim_step_kind)"""
    _fields_ = [(k, C.c_double) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "momentum", "rho", "alpha", "max_norm")] + \
               [(k, C.c_int) for k in ("kind", "nesterov", "sync")]


OPTIM_NOVOGRAD, OPTIM_SGD, OPTIM_ADADELTA = 0, 1, 2          # NSNP_OPTIM_* of include/nanosnp.h
OPTIM_MAX_TENSORS = 64


class OptimTensors:
    """The tensors of Context.optim_step, checked once (Context.optim_tensors): the five pointer tables, the counts, the scratch size"""
    __slots__ = ("n", "keep", "params", "grads", "exp_avg", "exp_avg_sq", "slow", "counts", "scratch_floats", "device", "grad_ptrs")


class Context:
    """One nsnp_ctx bound to one device (one per stream when batches overlap)."""

    def __init__(self, device=0, chunk_sites=None):
        import torch
        if not torch.cuda.is_available():
            raise NanoSNPError("no GPU visible: nanosnp_amd has no CPU fallback (the CPU restatement "
                               "under oracle/ is test infrastructure only)")
        self.lib = load()
        self.device = int(device)
        h = C.c_void_p()
        check(self.lib.nsnp_ctx_create(self.device, C.byref(h)), None, "nsnp_ctx_create")
        self.handle = h
        if chunk_sites:
            self.reserve(chunk_sites)

    def reserve(self, max_sites):
        check(self.lib.nsnp_ctx_reserve(self.handle, int(max_sites)), self.handle, "nsnp_ctx_reserve")

    def set_option(self, name, value):
        check(self.lib.nsnp_ctx_set_option(self.handle, name.encode(), int(value)), self.handle, f"nsnp_ctx_set_option({name})")

    # ids of nsnp_ctx_read_timing; the last three are ONE event pair around a chain of launches of a pass (include/nanosnp.h)
    KERNELS = ("pileup_l0", "pileup_proj1", "pileup_l1", "pileup_head", "encode_columns", "hap_features",
               "hap_lstm_chain", "cat_conv_chain", "cat_forward_pass", "hap_head", "train_forward", "train_backward", "train_wgrad",
               "hap_train_forward", "hap_train_backward", "hap_train_wgrad")

    def enable_timing(self, enable=True):
        check(self.lib.nsnp_ctx_enable_timing(self.handle, int(bool(enable))), self.handle, "nsnp_ctx_enable_timing")

    def read_timing(self):
        """{kernel name: (total_ms, launches)} of the launches recorded since the last read."""
        out = {}
        for k, name in enumerate(self.KERNELS):
            ms, n = C.c_double(0), C.c_int64(0)
            check(self.lib.nsnp_ctx_read_timing(self.handle, k, C.byref(ms), C.byref(n)), self.handle,
                  "nsnp_ctx_read_timing")
            out[name] = (ms.value, n.value)
        return out

    def shader_clock_mhz(self, stream=None):
        """shader clock under a ~2 ms full-chip fp32 MFMA load (diagnostic; bench lines record it)"""
        mhz = C.c_double(0)
        check(self.lib.nsnp_ctx_shader_clock(self.handle, C.byref(mhz), _stream_ptr(stream)), self.handle, "nsnp_ctx_shader_clock")
        return mhz.value

    def close(self):
        if getattr(self, "handle", None):
            self.lib.nsnp_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- optional RCCL gather of the C ABI (PyTorch ranks normally use nanosnp_amd.dist instead) ----
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * 128)()
        check(load().nsnp_comm_unique_id(buf), None, "nsnp_comm_unique_id")
        return bytes(buf)

    def comm_init(self, id128: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(id128)
        check(self.lib.nsnp_comm_init(self.handle, buf, int(rank), int(world)), self.handle, "nsnp_comm_init")
        self._comm = (int(rank), int(world))

    def gather_bytes(self, local, counts_bytes, root=0, stream=None):
        """local: contiguous cuda tensor of this rank; counts_bytes: bytes of every rank's block -> uint8 cuda tensor on root, else None"""
        import numpy as np
        import torch
        rank, world = self._comm
        off = np.concatenate([[0], np.cumsum(np.asarray(counts_bytes, np.int64))]).astype(np.int64)
        out = torch.empty(int(off[-1]), dtype=torch.uint8, device=local.device) if rank == root else None
        check(self.lib.nsnp_gather_results(self.handle, _dptr(local), int(local.numel() * local.element_size()), _dptr(out),
                                           off.ctypes.data_as(C.c_void_p), int(root), _stream_ptr(stream)), self.handle, "nsnp_gather_results")
        return out

    # ---- PileupModel -------------------------------------------------------------------------
    def pileup_load_weights(self, tensors):
        """tensors: 24 contiguous fp32 CPU arrays/tensors in state-dict order."""
        import numpy as np
        arrs = [np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
                for t in tensors]
        if len(arrs) < 24:
            raise NanoSNPError(f"expected 24 weight tensors, got {len(arrs)}")
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        check(self.lib.nsnp_pileup_load_weights(self.handle, ptrs, len(arrs)), self.handle,
              "nsnp_pileup_load_weights")

    def pileup_forward(self, x, gt=None, zy=None, stream=None):
        import torch
        assert x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and tuple(x.shape[1:]) == (33, 18)
        n = x.shape[0]
        gt = gt if gt is not None else torch.empty((n, 21), dtype=torch.float32, device=x.device)
        zy = zy if zy is not None else torch.empty((n, 3), dtype=torch.float32, device=x.device)
        check(self.lib.nsnp_pileup_forward(self.handle, _dptr(x), n, _dptr(gt), _dptr(zy), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_forward")
        return gt, zy

    def pileup_forward_windows(self, counts, center_idx, gt=None, zy=None, stream=None):
        import torch
        assert counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous()
        assert center_idx.is_cuda and center_idx.dtype == torch.int64 and center_idx.is_contiguous()
        n = center_idx.shape[0]
        gt = gt if gt is not None else torch.empty((n, 21), dtype=torch.float32, device=counts.device)
        zy = zy if zy is not None else torch.empty((n, 3), dtype=torch.float32, device=counts.device)
        check(self.lib.nsnp_pileup_forward_windows(self.handle, _dptr(counts), _dptr(center_idx), n, _dptr(gt),
                                                   _dptr(zy), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_forward_windows")
        return gt, zy

    def pileup_forward_windows_calls(self, counts, center_idx, stream=None, calls_out=None):
        """forward + argmax / max of both heads in one call -> (gt, zy, gt_arg, zy_arg, gt_max, zy_max).  calls_out = (gt_arg uint8 [n],
        zy_arg uint8 [n], gt_max float32 [n], zy_max float32 [n]): device tensors, or PINNED host tensors - the heads kernel then writes
        the 10 bytes per site straight into host memory (hipHostMalloc memory is mapped on the device) and no D2H copy is needed; they
        are valid on the host once an event recorded behind this call has completed."""
        import torch
        n = center_idx.shape[0]
        dev = counts.device
        gt = torch.empty((n, 21), dtype=torch.float32, device=dev); zy = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if calls_out is None:
            ga = torch.empty(n, dtype=torch.uint8, device=dev); za = torch.empty(n, dtype=torch.uint8, device=dev)
            gm = torch.empty(n, dtype=torch.float32, device=dev); zm = torch.empty(n, dtype=torch.float32, device=dev)
        else:
            ga, za, gm, zm = calls_out
            for t, dt in ((ga, torch.uint8), (za, torch.uint8), (gm, torch.float32), (zm, torch.float32)):
                if t.dtype != dt or t.numel() < n or not t.is_contiguous() or not (t.is_cuda or t.is_pinned()):
                    raise NanoSNPError("calls_out: contiguous uint8 / uint8 / float32 / float32 tensors of n elements, on the device or pinned")
        check(self.lib.nsnp_pileup_forward_windows_calls(self.handle, _dptr(counts), _dptr(center_idx), n, _dptr(gt), _dptr(zy), _dptr(ga),
                                                         _dptr(za), _dptr(gm), _dptr(zm), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_forward_windows_calls")
        return gt, zy, ga, za, gm, zm

    def pileup_rows_unpack(self, rows, outs, stream=None):
        """rows: device float64 [n,13] (pipeline.stream_contig); outs = (pos int64 [n], gt_arg uint8, zy_arg uint8, gt_max float32, zy_max
        float32, cov float32 [n,8]): device or PINNED host tensors of at least n elements - written by the kernel itself, no D2H copy; valid
        on the host once the stream has been synchronised."""
        import torch
        n = int(rows.shape[0])
        if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != 13 or not rows.is_contiguous() or not rows.is_cuda:
            raise NanoSNPError("rows: a contiguous device float64 [n,13] tensor")
        for t, dt, k in zip(outs, (torch.int64, torch.uint8, torch.uint8, torch.float32, torch.float32, torch.float32), (1, 1, 1, 1, 1, 8)):
            if t.dtype != dt or t.numel() < n * k or not t.is_contiguous() or not (t.is_cuda or t.is_pinned()):
                raise NanoSNPError("outs: contiguous int64 / uint8 / uint8 / float32 / float32 / float32 [n,8] tensors, on the device or pinned")
        check(self.lib.nsnp_pileup_rows_unpack(self.handle, _dptr(rows), n, *[_dptr(t) for t in outs], _stream_ptr(stream)),
              self.handle, "nsnp_pileup_rows_unpack")

    def pileup_postprocess(self, gt, zy, x=None, stream=None):
        import torch
        n = gt.shape[0]
        dev = gt.device
        gt_arg = torch.empty(n, dtype=torch.uint8, device=dev)
        zy_arg = torch.empty(n, dtype=torch.uint8, device=dev)
        gt_max = torch.empty(n, dtype=torch.float32, device=dev)
        zy_max = torch.empty(n, dtype=torch.float32, device=dev)
        depth = torch.empty(n, dtype=torch.int32, device=dev) if x is not None else None
        check(self.lib.nsnp_pileup_postprocess(self.handle, _dptr(gt), _dptr(zy), _dptr(x), n, _dptr(gt_arg),
                                               _dptr(zy_arg), _dptr(gt_max), _dptr(zy_max), _dptr(depth),
                                               _stream_ptr(stream)),
              self.handle, "nsnp_pileup_postprocess")
        return gt_arg, zy_arg, gt_max, zy_max, depth

    # ---- pileup encode -----------------------------------------------------------------------
    def pileup_encode_columns(self, bases, col_off, ref, min_af=0.12, min_coverage=6, stream=None, indel_min_af=None):
        """min_af: the SNP threshold and, unless indel_min_af is given, the indel threshold too (DNA_CreateCanSnpTensor -snp_min_af /
        -indel_min_af; make_predict_data.sh passes 0.12 for both)"""
        import torch
        assert bases.is_cuda and bases.dtype == torch.uint8 and col_off.dtype == torch.int64 and ref.dtype == torch.uint8
        m = ref.shape[0]
        dev = ref.device
        counts = torch.empty((m, 18), dtype=torch.int32, device=dev)
        depth = torch.empty(m, dtype=torch.int32, device=dev)
        flags = torch.empty(m, dtype=torch.uint8, device=dev)
        check(self.lib.nsnp_pileup_encode_columns2(self.handle, _dptr(bases), _dptr(col_off), _dptr(ref), m,
                                                   float(min_af), float(min_af if indel_min_af is None else indel_min_af), int(min_coverage),
                                                   _dptr(counts), _dptr(depth), _dptr(flags), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_encode_columns2")
        return counts, depth, flags

    def pileup_encode_columns3(self, bases, col_off, ref, pos=None, conf_bits=None, conf_n_bits=0, min_af=0.12, min_coverage=6, stream=None,
                               indel_min_af=None, want_max_del=True):
        """pileup_encode_columns with the confident BED and max_del_length (nsnp_pileup_encode_columns3) -> (counts, depth, flags, max_del
        int32 [M] or None).  conf_bits: device uint32 bitmap of the contig (bed.bed_bitmap), conf_n_bits its bits (the contig length); pos:
        device int64 [M], needed with a bitmap."""
        import torch
        assert bases.is_cuda and bases.dtype == torch.uint8 and col_off.dtype == torch.int64 and ref.dtype == torch.uint8
        m = ref.shape[0]
        dev = ref.device
        if conf_bits is not None:
            if conf_bits.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not conf_bits.is_cuda or not conf_bits.is_contiguous():
                raise NanoSNPError("conf_bits: a contiguous device tensor of 32-bit words")
            if conf_bits.numel() * 32 < int(conf_n_bits):
                raise NanoSNPError(f"conf_bits: {conf_bits.numel()} words hold fewer than conf_n_bits = {int(conf_n_bits)} bits")
        if pos is not None and (pos.dtype != torch.int64 or pos.shape[0] != m or not pos.is_contiguous()):
            raise NanoSNPError("pos: a contiguous int64 tensor of one position per column")
        counts = torch.empty((m, 18), dtype=torch.int32, device=dev)
        depth = torch.empty(m, dtype=torch.int32, device=dev)
        flags = torch.empty(m, dtype=torch.uint8, device=dev)
        max_del = torch.empty(m, dtype=torch.int32, device=dev) if want_max_del else None
        check(self.lib.nsnp_pileup_encode_columns3(self.handle, _dptr(bases), _dptr(col_off), _dptr(ref), _dptr(pos), m,
                                                   float(min_af), float(min_af if indel_min_af is None else indel_min_af), int(min_coverage),
                                                   _dptr(conf_bits), int(conf_n_bits), _dptr(counts), _dptr(depth), _dptr(flags), _dptr(max_del),
                                                   _stream_ptr(stream)),
              self.handle, "nsnp_pileup_encode_columns3")
        return counts, depth, flags, max_del

    FILTER_FRONT_PAD = 64     # readable bytes in front of the filtered bases (include/nanosnp.h: the encode of an all-empty wave reads 16)

    def pileup_filter_columns(self, pos, col_off, bases, ref, bits, n_bits, own_lo=0, own_hi=None, meta=None, out=None, stream=None):
        """The extended-BED stage (nsnp_pileup_filter_columns): the columns whose position p has bit p - 1 set, compacted, on the device ->
        (pos_out [M], off_out [M + 1], bases_out, ref_out [M], meta).  Entries behind the meta[0] kept columns are filled so that encode +
        select over all M make nothing of them.  meta: int64 [4] on the device or pinned = {K, kept bytes, kept columns in front of own_lo, of
        own_hi}; out: the four output tensors of an earlier call to reuse (capacities >= these inputs)."""
        import torch
        m = int(pos.shape[0])
        dev = pos.device
        own_hi = m if own_hi is None else own_hi
        nb = int(bases.numel())
        if bits is not None and (bits.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not bits.is_cuda or not bits.is_contiguous()):
            raise NanoSNPError("bits: a contiguous device tensor of 32-bit words")
        if bits is not None and bits.numel() * 32 < int(n_bits):
            raise NanoSNPError(f"bits: {bits.numel()} words hold fewer than n_bits = {int(n_bits)} bits")
        if col_off.shape[0] != m + 1 or ref.shape[0] != m:
            raise NanoSNPError("filter_columns: col_off [M + 1] and ref [M] must match pos [M]")
        if out is None:
            pad = self.FILTER_FRONT_PAD
            out = (torch.empty(max(m, 1), dtype=torch.int64, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev),
                   torch.empty(pad + max(nb, 1), dtype=torch.uint8, device=dev)[pad:], torch.empty(max(m, 1), dtype=torch.uint8, device=dev))
        po, oo, bo, ro = out
        if po.numel() < m or oo.numel() < m + 1 or bo.numel() < nb or ro.numel() < m:
            raise NanoSNPError("filter_columns: output buffers too small")
        meta = meta if meta is not None else torch.zeros(4, dtype=torch.int64, device=dev)
        check(self.lib.nsnp_pileup_filter_columns(self.handle, _dptr(pos), _dptr(col_off), _dptr(bases), _dptr(ref), m, _dptr(bits), int(n_bits),
                                                  int(own_lo), int(own_hi), _dptr(po), _dptr(oo), _dptr(bo), _dptr(ro), meta.data_ptr(),
                                                  _stream_ptr(stream)),
              self.handle, "nsnp_pileup_filter_columns")
        return po[:m], oo[:m + 1], bo[:max(nb, 1)], ro[:m], meta

    def pileup_filter_columns_keys(self, key, col_off, bases, ref, table, bed, aux=None, own_lo=0, own_hi=None, meta=None, out=None, stream=None):
        """pileup_filter_columns for the keyed columns of a whole-genome chunk (nsnp_pileup_filter_columns_keys): table the ContigTable of the
        keys, bed = (words, off) of a BedTable (its .ext); a column stays when the bit of its position is set in its OWN contig's bitmap.
        aux: device int32 [M] compacted with the columns (-1 behind the kept ones), or None -> (key_out [M], off_out [M + 1], bases_out,
        ref_out [M], aux_out [M] or None, meta).  out: the four (with aux: five) output tensors of an earlier call to reuse."""
        import torch
        m = int(key.shape[0])
        dev = key.device
        own_hi = m if own_hi is None else own_hi
        nb = int(bases.numel())
        words, off = _check_bed_pair(bed, table, "filter_columns_keys")
        if key.dtype != torch.int64 or not key.is_contiguous() or col_off.shape[0] != m + 1 or ref.shape[0] != m:
            raise NanoSNPError("filter_columns_keys: col_off [M + 1] and ref [M] must match the contiguous int64 key [M]")
        if aux is not None and (aux.dtype != torch.int32 or not aux.is_cuda or not aux.is_contiguous() or aux.numel() < m):
            raise NanoSNPError("filter_columns_keys: aux must be a contiguous device int32 tensor of at least M entries")
        if out is None:
            pad = self.FILTER_FRONT_PAD
            out = (torch.empty(max(m, 1), dtype=torch.int64, device=dev), torch.empty(m + 1, dtype=torch.int64, device=dev),
                   torch.empty(pad + max(nb, 1), dtype=torch.uint8, device=dev)[pad:], torch.empty(max(m, 1), dtype=torch.uint8, device=dev))
            if aux is not None:
                out += (torch.empty(max(m, 1), dtype=torch.int32, device=dev),)
        ko, oo, bo, ro = out[:4]
        ao = out[4] if aux is not None and len(out) > 4 else None
        if ko.numel() < m or oo.numel() < m + 1 or bo.numel() < nb or ro.numel() < m or (aux is not None and (ao is None or ao.numel() < m or ao.dtype != torch.int32)):
            raise NanoSNPError("filter_columns_keys: output buffers too small")
        meta = meta if meta is not None else torch.zeros(4, dtype=torch.int64, device=dev)
        check(self.lib.nsnp_pileup_filter_columns_keys(self.handle, _dptr(key), _dptr(col_off), _dptr(bases), _dptr(ref), _dptr(aux), m,
                                                       _dptr(words) if words.numel() else None, _dptr(off), _dptr(table.seq_off), len(table),
                                                       int(own_lo), int(own_hi), _dptr(ko), _dptr(oo), _dptr(bo), _dptr(ro), _dptr(ao),
                                                       meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_filter_columns_keys")
        return ko[:m], oo[:m + 1], bo[:max(nb, 1)], ro[:m], (ao[:m] if ao is not None else None), meta

    def pileup_encode_columns_keys(self, bases, col_off, ref, key=None, table=None, bed=None, min_af=0.12, min_coverage=6, stream=None,
                                   indel_min_af=None, want_max_del=True):
        """pileup_encode_columns3 for the keyed columns of a whole-genome chunk (nsnp_pileup_encode_columns_keys) -> (counts, depth, flags,
        max_del int32 [M] or None).  bed = (words, off) of a BedTable (its .conf) with table the ContigTable and key int64 [M]: a candidate
        then needs a set bit in [p - 1, p + max_del_length + 1) of its OWN contig; bed None: the candidates of pileup_encode_columns."""
        import torch
        assert bases.is_cuda and bases.dtype == torch.uint8 and col_off.dtype == torch.int64 and ref.dtype == torch.uint8
        m = ref.shape[0]
        dev = ref.device
        words = off = None
        if bed is not None:
            if table is None or key is None:
                raise NanoSNPError("encode_columns_keys: a bed table is tested at keys: key and table are needed")
            words, off = _check_bed_pair(bed, table, "encode_columns_keys")
        if key is not None and (key.dtype != torch.int64 or key.shape[0] != m or not key.is_contiguous()):
            raise NanoSNPError("key: a contiguous int64 tensor of one key per column")
        counts = torch.empty((m, 18), dtype=torch.int32, device=dev)
        depth = torch.empty(m, dtype=torch.int32, device=dev)
        flags = torch.empty(m, dtype=torch.uint8, device=dev)
        max_del = torch.empty(m, dtype=torch.int32, device=dev) if want_max_del else None
        check(self.lib.nsnp_pileup_encode_columns_keys(self.handle, _dptr(bases), _dptr(col_off), _dptr(ref), _dptr(key), m,
                                                       float(min_af), float(min_af if indel_min_af is None else indel_min_af), int(min_coverage),
                                                       _dptr(words) if words is not None and words.numel() else None, _dptr(off),
                                                       _dptr(table.seq_off) if table is not None else None, len(table) if table is not None else 0,
                                                       _dptr(counts), _dptr(depth), _dptr(flags), _dptr(max_del), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_encode_columns_keys")
        return counts, depth, flags, max_del

    def pileup_select_sites_range_dev(self, pos, flags, own, meta, stream=None):
        """pileup_select_sites_range with the bounds {own_lo, own_hi} read from `own` (int64 [2], device or pinned: e.g. meta[2:] of
        pileup_filter_columns) when the launches run"""
        import torch
        m = pos.shape[0]
        center = torch.empty(max(m, 1), dtype=torch.int64, device=pos.device)
        if own.dtype != torch.int64 or own.numel() < 2 or not (own.is_cuda or own.is_pinned()):
            raise NanoSNPError("own: int64 [2] on the device or pinned")
        check(self.lib.nsnp_pileup_select_sites_range_dev(self.handle, _dptr(pos), _dptr(flags), m, own.data_ptr(), _dptr(center), m,
                                                          meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_select_sites_range_dev")
        return center

    def pileup_select_sites(self, pos, flags, cap=None, stream=None):
        import torch
        m = pos.shape[0]
        cap = int(cap if cap is not None else m)
        center = torch.empty(max(cap, 1), dtype=torch.int64, device=pos.device)
        n_sites = torch.zeros(1, dtype=torch.int64, device=pos.device)
        check(self.lib.nsnp_pileup_select_sites(self.handle, _dptr(pos), _dptr(flags), m, _dptr(center), cap,
                                                _dptr(n_sites), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_select_sites")
        n = int(n_sites.item())
        return center[:min(n, cap)], n

    def pileup_select_sites_async(self, pos, flags, stream=None):
        """select_sites without the host round trip: -> (center_idx int64 [M], entries behind the selected ones = 2^62; n_sites: device
        int64 [1]).  The streamed pipeline reads the count through a pinned buffer one chunk later (nanosnp_amd/pipeline.py)."""
        import torch
        m = pos.shape[0]
        center = torch.full((max(m, 1),), 1 << 62, dtype=torch.int64, device=pos.device)
        n_sites = torch.zeros(1, dtype=torch.int64, device=pos.device)
        check(self.lib.nsnp_pileup_select_sites(self.handle, _dptr(pos), _dptr(flags), m, _dptr(center), m,
                                                _dptr(n_sites), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_select_sites")
        return center, n_sites

    TOK_EFORMAT, TOK_BLANK, TOK_EPOS, TOK_ERANGE = 1, 2, 4, 8

    def mpileup_tokenise_into(self, text, chr_seq, pos, col_off, bases, ref, meta, stream=None):
        """nsnp_mpileup_tokenise into the caller's buffers, asynchronously: text uint8 [T] on the device; chr_seq uint8 on the device (or
        None, with ref None); pos int64 [cap], col_off int64 [cap + 1], bases uint8 [cap_bytes], ref uint8 [cap] on the device; meta int64 [4]
        on the device or in pinned host memory ({lines, bytes, status, 0} once the stream has passed the call)."""
        check(self.lib.nsnp_mpileup_tokenise(self.handle, _dptr(text), int(text.numel()), _dptr(chr_seq) if chr_seq is not None else None,
                                             int(chr_seq.numel()) if chr_seq is not None else 0, int(pos.numel()), int(bases.numel()),
                                             _dptr(pos), _dptr(col_off), _dptr(bases), _dptr(ref) if ref is not None else None,
                                             meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_mpileup_tokenise")

    def mpileup_tokenise(self, text, chr_seq=None, stream=None):
        """mpileup text (uint8 device tensor) -> (pos [M] int64, col_off [M + 1] int64, bases uint8, ref uint8 [M] or None) on the device.
        Synchronous (the sizes come back from the device, read behind `stream`); raises on text the reference's reader could not read."""
        import torch
        dev = text.device
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        t = int(text.numel())
        cap, cap_b = t // 10 + 2, max(t, 1)
        while True:
            with torch.cuda.stream(s):                 # (the outputs belong to the stream that writes them)
                pos = torch.empty(cap, dtype=torch.int64, device=dev)
                off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
                bases = torch.empty(cap_b, dtype=torch.uint8, device=dev)
                ref = torch.empty(cap, dtype=torch.uint8, device=dev) if chr_seq is not None else None
                meta = torch.zeros(4, dtype=torch.int64, device=dev)
                self.mpileup_tokenise_into(text, chr_seq, pos, off, bases, ref, meta, s)
                m, nb, status, _ = meta.tolist()       # (the read is queued on `s`, behind the kernels)
            if status & self.TOK_ERANGE and not status & (self.TOK_EFORMAT | self.TOK_BLANK):
                if (cap, cap_b) == (max(cap, m + 1), max(cap_b, nb)):
                    break
                cap, cap_b = max(cap, m + 1), max(cap_b, nb)
                continue
            break
        tokenise_status_check(status)
        torch.cuda.current_stream(dev).wait_stream(s)
        return pos[:m], off[:m + 1], bases[:nb], (ref[:m] if ref is not None else None)

    TOK_ENAME = 16

    def mpileup_tokenise_contigs_into(self, text, table, pos, col_off, bases, ref, cid, key, runs, meta, stream=None):
        """nsnp_mpileup_tokenise_contigs into the caller's buffers, asynchronously: text uint8 [T] on the device, table a ContigTable; pos
        int64 [cap], col_off int64 [cap + 1], bases uint8 [cap_bytes], ref uint8 [cap], cid int32 [cap], key int64 [cap] on the device; runs
        int64 [cap_runs, 2] and meta int64 [4] on the device or in pinned host memory ({lines, bytes, status, runs} once the stream has
        passed the call)."""
        check(self.lib.nsnp_mpileup_tokenise_contigs(self.handle, _dptr(text), int(text.numel()), _dptr(table.names_blob), _dptr(table.name_off),
                                                     _dptr(table.genome), _dptr(table.seq_off), len(table), int(table.genome_len),
                                                     int(min(pos.numel(), ref.numel(), cid.numel(), key.numel())), int(bases.numel()),
                                                     int(runs.numel() // 2), _dptr(pos), _dptr(col_off), _dptr(bases), _dptr(ref), _dptr(cid),
                                                     _dptr(key), runs.data_ptr(), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_mpileup_tokenise_contigs")

    def mpileup_tokenise_contigs(self, text, table, stream=None):
        """mpileup text of several contigs (uint8 device tensor) -> (pos [M] int64, col_off [M + 1] int64, bases uint8, ref uint8 [M], cid int32
        [M], key int64 [M], runs int64 [R, 2]) on the device.  Synchronous (the sizes come back from the device, read behind `stream`);
        raises on text the reference's reader could not read."""
        import torch
        s = stream if stream is not None else torch.cuda.current_stream(text.device)
        t = int(text.numel())
        cap, cap_b, cap_r = t // 10 + 2, max(t, 1), 1024
        dev = text.device
        while True:
            with torch.cuda.stream(s):                 # (the outputs belong to the stream that writes them)
                pos = torch.empty(cap, dtype=torch.int64, device=dev)
                off = torch.empty(cap + 1, dtype=torch.int64, device=dev)
                bases = torch.empty(cap_b, dtype=torch.uint8, device=dev)
                ref = torch.empty(cap, dtype=torch.uint8, device=dev)
                cid = torch.empty(cap, dtype=torch.int32, device=dev)
                key = torch.empty(cap, dtype=torch.int64, device=dev)
                runs = torch.empty((cap_r, 2), dtype=torch.int64, device=dev)
                meta = torch.zeros(4, dtype=torch.int64, device=dev)
                self.mpileup_tokenise_contigs_into(text, table, pos, off, bases, ref, cid, key, runs, meta, s)
                m, nb, status, r = meta.tolist()       # (the read is queued on `s`, behind the kernels)
            if status & self.TOK_ERANGE and not status & (self.TOK_EFORMAT | self.TOK_BLANK | self.TOK_ENAME):
                if (cap, cap_b, cap_r) == (max(cap, m + 1), max(cap_b, nb), max(cap_r, r)):
                    break
                cap, cap_b, cap_r = max(cap, m + 1), max(cap_b, nb), max(cap_r, r)
                continue
            break
        tokenise_status_check(status)
        torch.cuda.current_stream(dev).wait_stream(s)
        return pos[:m], off[:m + 1], bases[:nb], ref[:m], cid[:m], key[:m], runs[:r]

    def pileup_select_sites_range(self, pos, flags, own_lo, own_hi, meta, stream=None):
        """select_sites for one chunk of a streamed text, without a host round trip: -> center_idx int64 [M] (the first meta[0] entries are the
        selected centres, ascending); meta (int64 [4], on the device or pinned) receives {n, c_lo, c_hi, n}: the chunk's own sites - centres in
        [own_lo, own_hi) - are center_idx[c_lo:c_hi]."""
        import torch
        m = pos.shape[0]
        center = torch.empty(max(m, 1), dtype=torch.int64, device=pos.device)
        check(self.lib.nsnp_pileup_select_sites_range(self.handle, _dptr(pos), _dptr(flags), m, int(own_lo), int(own_hi), _dptr(center), m,
                                                      meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_select_sites_range")
        return center

    def pileup_call_rows(self, counts, center_idx, pos, gt_arg, zy_arg, gt_max, zy_max, stream=None):
        """-> the call rows [n,13] float64 of the text pipeline (position, argmax / max of both heads, the eight coverage channels of
        predict.py:63 at the centre column) in one launch"""
        import torch
        n = int(center_idx.shape[0])
        rows = torch.empty((n, 13), dtype=torch.float64, device=counts.device)
        check(self.lib.nsnp_pileup_call_rows(self.handle, _dptr(counts), _dptr(center_idx), _dptr(pos), _dptr(gt_arg), _dptr(zy_arg), _dptr(gt_max),
                                             _dptr(zy_max), n, _dptr(rows), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_call_rows")
        return rows

    POSITION_WIDTH = 83       # NSNP_POSITION_WIDTH = sitefile.POSITION_WIDTH

    NAME_ENTRY = 44           # NSNP_NAME_ENTRY

    # ---- what the wrappers of the record entries share (one contig: pos + chr_seq + name; several: key + ContigTable) ----

    @staticmethod
    def _device_or_pinned(*outs):
        for t, what in outs:
            if not (t.is_cuda or t.is_pinned()) or not t.is_contiguous():
                raise NanoSNPError(f"{what}: a contiguous tensor on the device or in pinned memory")

    def _line_names_outputs(self, text, cap_lines, cap_names, line_idx, names, meta):
        """line_idx, names and meta of mpileup_line_names / _contigs: those not given, then the checks"""
        import torch
        dev = text.device
        if line_idx is None:
            line_idx = torch.empty(max(int(cap_lines), 1), dtype=torch.int32, device=dev)
        if names is None:
            names = torch.empty((max(int(cap_names), 1), self.NAME_ENTRY), dtype=torch.uint8, device=dev)
        if meta is None:
            meta = torch.zeros(4, dtype=torch.int64, device=dev)
        assert text.dtype == torch.uint8 and text.is_cuda and line_idx.dtype == torch.int32 and line_idx.is_cuda and names.is_cuda
        return line_idx, names, meta

    def _records_outputs(self, what, n, elem, dev, position_matrix, position, meta, site_key=False):
        """The outputs of pileup_window_records / _keys: those not given, then the checks (site_key False: the entry has none)"""
        import torch
        dt = {2: torch.int16, 4: torch.int32}.get(elem)
        if dt is None:
            raise NanoSNPError("elem: 2 (int16) or 4 (int32)")
        keyed = site_key is not False
        if position_matrix is None:
            position_matrix = torch.empty((max(n, 1), 33, 18), dtype=dt, device=dev)
        if position is None:
            position = torch.empty((max(n, 1), self.POSITION_WIDTH), dtype=torch.uint8, device=dev)
        if keyed and site_key is None:
            site_key = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        if meta is None:
            meta = torch.zeros(4, dtype=torch.int64, device=dev)
        self._device_or_pinned((position_matrix, "position_matrix"), (position, "position"), *([(site_key, "site_key")] if keyed else []), (meta, "meta"))
        if (position_matrix.dtype != dt or position_matrix.numel() < n * 594 or position.dtype != torch.uint8 or position.numel() < n * self.POSITION_WIDTH
                or (keyed and (site_key.dtype != torch.int64 or site_key.numel() < n))):
            raise NanoSNPError(f"{what}: output buffers too small or of the wrong type")
        return position_matrix, position, site_key, meta

    def _records_views(self, n, position_matrix, position):
        return position_matrix.view(-1)[:n * 594].view(n, 33, 18), position.view(-1)[:n * self.POSITION_WIDTH].view(n, self.POSITION_WIDTH)

    @staticmethod
    def _line_names_arg(line_names, m, maker):
        """(line_idx, names) of `maker` for the same lines, or (None, None): per-site names"""
        import torch
        line_idx, names = line_names if line_names is not None else (None, None)
        if line_idx is not None and (line_idx.dtype != torch.int32 or line_idx.numel() < m or not line_idx.is_cuda or not names.is_cuda):
            raise NanoSNPError(f"line_names: device int32 [M] and the name table of {maker}")
        return line_idx, names

    def _alt_info_run(self, what, launch, n, dev, cap, blob, offsets, meta, stream):
        """The outputs of pileup_alt_info / _keys (those not given, then the checks), launch(blob, cap, offsets, meta), and the second run
        with the size the first one reported when neither a cap nor a blob was given"""
        import torch
        retry = cap is None and blob is None
        cap = int(blob.numel() if blob is not None else (64 * n + 4096 if cap is None else cap))
        if blob is None:
            blob = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
        if offsets is None:
            offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        if meta is None:
            meta = torch.zeros(4, dtype=torch.int64, device=dev)
        self._device_or_pinned((blob, "blob"), (offsets, "offsets"), (meta, "meta"))
        if blob.numel() < cap or offsets.numel() < n + 1:
            raise NanoSNPError(f"{what}: output buffers too small")
        launch(blob, cap, offsets, meta)
        if retry:
            (stream or torch.cuda.current_stream(dev)).synchronize()
            need = int(meta[0])
            if need > cap:
                return self._alt_info_run(what, launch, n, dev, need, None, offsets, meta, stream)
        return blob, offsets[:n + 1], meta

    def mpileup_line_names(self, text, name, cap_lines, cap_names=64, line_idx=None, names=None, meta=None, stream=None):
        """Column 0 of every line of a device text against `name` (nsnp_mpileup_line_names) -> (line_idx int32 [cap_lines]: -1 where the
        line's first token is `name`, else its entry in names; names uint8 [cap_names, 44]; meta int64 [4] = {lines that differ, status})"""
        name = name.encode() if isinstance(name, str) else bytes(name)
        line_idx, names, meta = self._line_names_outputs(text, cap_lines, cap_names, line_idx, names, meta)
        check(self.lib.nsnp_mpileup_line_names(self.handle, _dptr(text), int(text.numel()), name, len(name), int(line_idx.numel()), _dptr(line_idx),
                                               _dptr(names), int(names.shape[0]), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_mpileup_line_names")
        return line_idx, names, meta

    def pileup_window_records(self, counts, center_idx, pos, chr_seq, name, elem=2, position_matrix=None, position=None, meta=None, stream=None,
                              line_names=None):
        """The first two arrays of a .pd.bin for the sites center_idx [N] of a chunk (nsnp_pileup_window_records) -> (position_matrix
        [N,33,18] int16 / int32 for elem 2 / 4, position uint8 [N,83], meta int64 [4] = {N, int16 overflow, status, 0}).  counts int32 [M,18],
        pos int64 [M], chr_seq uint8: device tensors; name: the contig name (str or bytes).  The three outputs may be given: device or
        pinned tensors with room for N sites (the first N rows are written); meta is valid once the stream has passed the call."""
        import torch
        n, m = int(center_idx.shape[0]), int(counts.shape[0])
        assert counts.dtype == torch.int32 and center_idx.dtype == torch.int64 and pos.dtype == torch.int64 and chr_seq.dtype == torch.uint8
        name = name.encode() if isinstance(name, str) else bytes(name)
        position_matrix, position, _, meta = self._records_outputs("window_records", n, elem, counts.device, position_matrix, position, meta)
        line_idx, names = self._line_names_arg(line_names, m, "mpileup_line_names")
        check(self.lib.nsnp_pileup_window_records2(self.handle, _dptr(counts), _dptr(center_idx), _dptr(pos), m, n, _dptr(chr_seq), int(chr_seq.numel()),
                                                   name, len(name), int(elem), _dptr(line_idx), _dptr(names), position_matrix.data_ptr(),
                                                   position.data_ptr(), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_window_records2")
        return (*self._records_views(n, position_matrix, position), meta)

    def pileup_alt_info(self, bases, col_off, ref, pos, depth, center_idx, chr_seq, cap=None, blob=None, offsets=None, meta=None, stream=None):
        """The alt_info texts of the sites center_idx [N] (nsnp_pileup_alt_info) -> (blob uint8 [cap], offsets int64 [N + 1], meta int64 [4] =
        {bytes needed, status, 0, 0}); text n is blob[offsets[n]:offsets[n + 1]].  status has TOK_ERANGE when needed > cap (the blob is then
        untouched).  blob / offsets / meta may be given (device or pinned); without a cap the call waits and runs again when the first
        guess was too small."""
        import torch
        n, m = int(center_idx.shape[0]), int(ref.shape[0])
        assert bases.dtype == torch.uint8 and col_off.dtype == torch.int64 and ref.dtype == torch.uint8 and pos.dtype == torch.int64
        assert depth.dtype == torch.int32 and center_idx.dtype == torch.int64 and chr_seq.dtype == torch.uint8
        if col_off.shape[0] != m + 1 or pos.shape[0] != m or depth.shape[0] != m:
            raise NanoSNPError("alt_info: col_off [M + 1], pos [M] and depth [M] must match ref [M]")

        def launch(blob, cap, offsets, meta):
            check(self.lib.nsnp_pileup_alt_info(self.handle, _dptr(bases), int(bases.numel()), _dptr(col_off), _dptr(ref), _dptr(pos), _dptr(depth), m,
                                                _dptr(center_idx), n, _dptr(chr_seq), int(chr_seq.numel()), blob.data_ptr(), cap, offsets.data_ptr(),
                                                meta.data_ptr(), _stream_ptr(stream)),
                  self.handle, "nsnp_pileup_alt_info")
        return self._alt_info_run("alt_info", launch, n, ref.device, cap, blob, offsets, meta, stream)

    def mpileup_line_names_contigs(self, text, cid, table, cap_lines=None, cap_names=64, line_idx=None, names=None, meta=None, stream=None):
        """mpileup_line_names against a ContigTable (nsnp_mpileup_line_names_contigs): cid int32 per line as mpileup_tokenise_contigs wrote it
        for the same device text -> (line_idx int32 [cap_lines]: -1 where the line's first token is the table name of its contig or the line
        belongs to no wanted contig, else its entry in names; names uint8 [cap_names, 44]; meta int64 [4] = {lines that differ, status})"""
        import torch
        cap_lines = int(cid.numel() if cap_lines is None else cap_lines)
        line_idx, names, meta = self._line_names_outputs(text, cap_lines, cap_names, line_idx, names, meta)
        if cid.dtype != torch.int32 or not cid.is_cuda or not cid.is_contiguous() or cid.numel() < cap_lines or line_idx.numel() < cap_lines:
            raise NanoSNPError("line_names_contigs: cid and line_idx must be contiguous device int32 tensors of at least cap_lines entries")
        check(self.lib.nsnp_mpileup_line_names_contigs(self.handle, _dptr(text), int(text.numel()), _dptr(cid), _dptr(table.names_blob),
                                                       _dptr(table.name_off), len(table), cap_lines, _dptr(line_idx), _dptr(names),
                                                       int(names.shape[0]), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_mpileup_line_names_contigs")
        return line_idx, names, meta

    def pileup_window_records_keys(self, counts, center_idx, key, table, elem=2, position_matrix=None, position=None, site_key=None, meta=None,
                                   stream=None, line_names=None, cap_names=None):
        """pileup_window_records for a chunk of several contigs (nsnp_pileup_window_records_keys): key int64 [M] as mpileup_tokenise_contigs
        wrote it, table the ContigTable of that call -> (position_matrix [N,33,18], position uint8 [N,83], site_key int64 [N] = key[centre],
        meta int64 [4] = {N, int16 overflow, status, 0}).  line_names: (line_idx, names) of mpileup_line_names_contigs for the same lines;
        cap_names: the entries of names that count (default: all it holds).  The four outputs may be given: device or pinned tensors."""
        import torch
        n, m = int(center_idx.shape[0]), int(counts.shape[0])
        assert counts.dtype == torch.int32 and center_idx.dtype == torch.int64 and key.dtype == torch.int64
        if key.shape[0] != m or not key.is_contiguous():
            raise NanoSNPError("window_records_keys: key [M] must match counts [M,18]")
        position_matrix, position, site_key, meta = self._records_outputs("window_records_keys", n, elem, counts.device, position_matrix, position, meta,
                                                                          site_key)
        line_idx, names = self._line_names_arg(line_names, m, "mpileup_line_names_contigs")
        n_names = int(names.numel() // self.NAME_ENTRY) if names is not None else 0
        cap_names = n_names if cap_names is None else int(cap_names)
        if cap_names < 0 or cap_names > n_names:
            raise NanoSNPError("window_records_keys: cap_names beyond the name table")
        check(self.lib.nsnp_pileup_window_records_keys(self.handle, _dptr(counts), _dptr(center_idx), _dptr(key), m, n, _dptr(table.names_blob),
                                                       _dptr(table.name_off), _dptr(table.genome), _dptr(table.seq_off), len(table), int(elem),
                                                       _dptr(line_idx), _dptr(names), cap_names, position_matrix.data_ptr(), position.data_ptr(),
                                                       site_key.data_ptr(), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_window_records_keys")
        return (*self._records_views(n, position_matrix, position), site_key.view(-1)[:n], meta)

    def pileup_alt_info_keys(self, bases, col_off, ref, key, depth, center_idx, table, cap=None, blob=None, offsets=None, meta=None, stream=None):
        """pileup_alt_info for a chunk of several contigs (nsnp_pileup_alt_info_keys): key int64 [M] for pos, the ContigTable for chr_seq -> (blob
        uint8 [cap], offsets int64 [N + 1], meta int64 [4] = {bytes needed, status, 0, 0}); everything else as pileup_alt_info."""
        import torch
        n, m = int(center_idx.shape[0]), int(ref.shape[0])
        assert bases.dtype == torch.uint8 and col_off.dtype == torch.int64 and ref.dtype == torch.uint8 and key.dtype == torch.int64
        assert depth.dtype == torch.int32 and center_idx.dtype == torch.int64
        if col_off.shape[0] != m + 1 or key.shape[0] != m or depth.shape[0] != m:
            raise NanoSNPError("alt_info_keys: col_off [M + 1], key [M] and depth [M] must match ref [M]")

        def launch(blob, cap, offsets, meta):
            check(self.lib.nsnp_pileup_alt_info_keys(self.handle, _dptr(bases), int(bases.numel()), _dptr(col_off), _dptr(ref), _dptr(key), _dptr(depth), m,
                                                     _dptr(center_idx), n, _dptr(table.genome), _dptr(table.seq_off), len(table), blob.data_ptr(), cap,
                                                     offsets.data_ptr(), meta.data_ptr(), _stream_ptr(stream)),
                  self.handle, "nsnp_pileup_alt_info_keys")
        return self._alt_info_run("alt_info_keys", launch, n, ref.device, cap, blob, offsets, meta, stream)

    LABEL_WIDTH = 90

    def pileup_label_sites_keys(self, key, center_idx, table, truth_key, truth_code, keep_thr=None, seed=0, out_center_idx=None, label=None,
                                counts=None, meta=None, stream=None, want_label=True):
        """The training labels of a chunk's selected sites (nsnp_pileup_label_sites_keys): key int64 [M] as mpileup_tokenise_contigs wrote it,
        center_idx int64 [N], table the ContigTable of that call, truth_key device int64 [T] ascending / truth_code device int32 [T] (the
        packed codes of truth.load_truth, as int32 bits), keep_thr device int64 [n_contigs] (thresholds below 2^63) or None: every site is
        kept -> (out_center_idx int64 [N] on the device: the first N' entries are the kept centres in order, label int32 [N, 90]: the first
        N' rows are theirs, meta int64 [4] = {N', truth sites, other sites, status}).  N' is only known behind the launch: the caller reads
        it from meta.  want_label=False (count mode): no label and no centre is written; counts: device int64 [n_contigs, 2] to which the
        chunk's {truth sites, other sites} per contig are added.  label and meta may be given: device or pinned tensors."""
        import torch
        n, m = int(center_idx.shape[0]), int(key.shape[0])
        dev = key.device
        for t, dt, what in ((key, torch.int64, "key"), (center_idx, torch.int64, "center_idx"), (truth_key, torch.int64, "truth_key"),
                            (truth_code, torch.int32, "truth_code"), (keep_thr, torch.int64, "keep_thr"), (counts, torch.int64, "counts"),
                            (out_center_idx, torch.int64, "out_center_idx")):
            if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
                raise NanoSNPError(f"label_sites_keys: {what} must be a contiguous device tensor of {dt}")
        if truth_code.numel() != truth_key.numel():
            raise NanoSNPError("label_sites_keys: one truth_code per truth_key")
        if (keep_thr is not None and keep_thr.numel() != len(table)) or (counts is not None and counts.numel() != 2 * len(table)):
            raise NanoSNPError("label_sites_keys: keep_thr [n_contigs] and counts [n_contigs, 2] belong to the contig table")
        if meta is None:
            meta = torch.zeros(4, dtype=torch.int64, device=dev)
        if want_label:
            if out_center_idx is None:
                out_center_idx = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
            if label is None:
                label = torch.empty((max(n, 1), self.LABEL_WIDTH), dtype=torch.int32, device=dev)
            if label.dtype != torch.int32 or label.numel() < n * self.LABEL_WIDTH or out_center_idx.numel() < n:
                raise NanoSNPError("label_sites_keys: output buffers too small or of the wrong type")
        else:
            out_center_idx = label = None
        for t, what in ((label, "label"), (meta, "meta")):
            if t is not None and (not (t.is_cuda or t.is_pinned()) or not t.is_contiguous()):
                raise NanoSNPError(f"{what}: a contiguous tensor on the device or in pinned memory")
        if meta.dtype != torch.int64 or meta.numel() < 4:
            raise NanoSNPError("label_sites_keys: meta int64 [4]")
        check(self.lib.nsnp_pileup_label_sites_keys(self.handle, _dptr(key), m, _dptr(center_idx), n, _dptr(table.genome), _dptr(table.seq_off),
                                                    len(table), _dptr(truth_key), _dptr(truth_code), int(truth_key.numel()), _dptr(keep_thr),
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, _dptr(out_center_idx), _dptr(label), _dptr(counts),
                                                    meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_label_sites_keys")
        if not want_label:
            return None, None, meta
        return out_center_idx.view(-1)[:n], label.view(-1)[:n * self.LABEL_WIDTH].view(n, self.LABEL_WIDTH), meta

    # ---- scoring on labelled windows (include/nanosnp.h; fp32 only) ----
    EVAL_COUNTERS = 2628
    EVAL_HEADS = ((0, 21, 0), (21, 3, 441), (24, 33, 450), (57, 33, 1539))      # (first head row, classes, first counter) of gt, zy, id1, id2

    def pileup_load_indel_heads(self, tensors):
        """tensors: indel1_layer.weight [33,256], .bias [33], indel2_layer.weight [33,256], .bias [33]; after pileup_load_weights"""
        import numpy as np
        arrs = [np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32) for t in tensors]
        if [a.shape for a in arrs] != [(33, 256), (33,), (33, 256), (33,)]:
            raise NanoSNPError(f"expected the four indel tensors [33,256], [33], [33,256], [33], got {[a.shape for a in arrs]}")
        ptrs = (C.c_void_p * 4)(*[a.ctypes.data for a in arrs])
        check(self.lib.nsnp_pileup_load_indel_heads(self.handle, ptrs, 4), self.handle, "nsnp_pileup_load_indel_heads")

    def pileup_label_classes(self, label, variants_only=True, cls=None, center_idx=None, meta=None, stream=None):
        """label: device int32 [N,90] -> (cls uint8 [N,4], center_idx int64 [N], meta int64 [4]): the first meta[0] rows of cls / center_idx
        are the kept rows' classes {gt, zy, id1, id2} and centres 33 n + 16, in order; meta[1] = rows that are not one-hot in some family.
        meta may be pinned host memory; the count is only known behind the launch."""
        import torch
        if label.dtype != torch.int32 or not label.is_cuda or not label.is_contiguous() or label.dim() != 2 or label.shape[1] != self.LABEL_WIDTH:
            raise NanoSNPError(f"label_classes: label must be a contiguous device int32 [N,{self.LABEL_WIDTH}]")
        n, dev = int(label.shape[0]), label.device
        cls = cls if cls is not None else torch.empty((max(n, 1), 4), dtype=torch.uint8, device=dev)
        center_idx = center_idx if center_idx is not None else torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        meta = meta if meta is not None else torch.zeros(4, dtype=torch.int64, device=dev)
        if (cls.dtype != torch.uint8 or cls.numel() < 4 * n or not cls.is_cuda or not cls.is_contiguous() or center_idx.dtype != torch.int64
                or center_idx.numel() < n or not center_idx.is_cuda or not center_idx.is_contiguous()):
            raise NanoSNPError("label_classes: cls uint8 [N,4] and center_idx int64 [N] on the device")
        if meta.dtype != torch.int64 or meta.numel() < 4 or not (meta.is_cuda or meta.is_pinned()) or not meta.is_contiguous():
            raise NanoSNPError("label_classes: meta int64 [4] on the device or in pinned memory")
        check(self.lib.nsnp_pileup_label_classes(self.handle, _dptr(label), n, int(bool(variants_only)), _dptr(cls), _dptr(center_idx),
                                                 meta.data_ptr(), _stream_ptr(stream)), self.handle, "nsnp_pileup_label_classes")
        return cls, center_idx, meta

    def pileup_balance_samples(self, cls, n, seed, draw=0, samples=None, sizes=None, meta=None, stream=None):
        """cls: device uint8 [>= n, 4] as pileup_label_classes leaves it -> (samples int64, sizes int64 [63] or None, meta int64 [8]): the
        training sample list of a pass under balance_dataset upsampling (nsnp_pileup_balance_samples): the first meta[0] entries of samples
        are row indices in [0, n); sizes = the rows per (genotype, zygosity) category 3 gt + zy; meta = {M, K, U, max, rows in no category,
        status, 0, 0}, on the device or in pinned memory.  status 1 (U == 0: no category below the largest): M = 0 and no sample is
        written.  seed: 64 bits, draw: 32 bits (the pass counter).  samples None: a new tensor of 2 n entries, which always suffices; a
        given one smaller than M is refused with nothing written.  sizes None: a new tensor; False: not wanted (NULL).  The entry waits for
        the stream once (for M)."""
        import torch
        n, seed, draw = int(n), int(seed), int(draw)
        if cls.dtype != torch.uint8 or not cls.is_cuda or not cls.is_contiguous() or n < 0 or cls.numel() < 4 * n:
            raise NanoSNPError("pileup_balance_samples: cls must be a contiguous device uint8 [n,4]")
        if n >= 1 << 32:
            raise NanoSNPError("pileup_balance_samples: n below 2^32")
        if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
            raise NanoSNPError("pileup_balance_samples: seed in [0, 2^64) and draw in [0, 2^32)")
        dev = cls.device
        if samples is None:
            samples = torch.empty(max(2 * n, 1), dtype=torch.int64, device=dev)
        if sizes is None:
            sizes = torch.zeros(63, dtype=torch.int64, device=dev)
        elif sizes is False:
            sizes = None
        meta = meta if meta is not None else torch.zeros(8, dtype=torch.int64, device=dev)
        if samples.dtype != torch.int64 or not samples.is_cuda or not samples.is_contiguous():
            raise NanoSNPError("pileup_balance_samples: samples int64 on the device")
        if sizes is not None and (sizes.dtype != torch.int64 or sizes.numel() < 63 or not sizes.is_cuda or not sizes.is_contiguous()):
            raise NanoSNPError("pileup_balance_samples: sizes int64 [63] on the device")
        if meta.dtype != torch.int64 or meta.numel() < 8 or not (meta.is_cuda or meta.is_pinned()) or not meta.is_contiguous():
            raise NanoSNPError("pileup_balance_samples: meta int64 [8] on the device or in pinned memory")
        check(self.lib.nsnp_pileup_balance_samples(self.handle, _dptr(cls), n, seed, draw, _dptr(samples), int(samples.numel()), _dptr(sizes),
                                                   meta.data_ptr(), _stream_ptr(stream)), self.handle, "nsnp_pileup_balance_samples")
        return samples, sizes, meta

    @staticmethod
    def _eval_inputs(counts, center_idx, what):
        import torch
        if counts.dtype != torch.int32 or not counts.is_cuda or not counts.is_contiguous():
            raise NanoSNPError(f"{what}: counts must be a contiguous device int32 tensor")
        if center_idx is None:
            if counts.dim() != 3 or tuple(counts.shape[1:]) != (33, 18):
                raise NanoSNPError(f"{what}: without center_idx counts is [N,33,18]")
            return int(counts.shape[0])
        if center_idx.dtype != torch.int64 or not center_idx.is_cuda or not center_idx.is_contiguous():
            raise NanoSNPError(f"{what}: center_idx must be a contiguous device int64 tensor")
        return int(center_idx.shape[0])

    @staticmethod
    def eval_precision_arg(precision):
        """the `precision` keyword of the scoring calls -> None (the fp32-only entry, which refuses while pileup_precision is 1 or 2) or the
        argument of the numbered entries: 0 fp32, 1 f16x3, 2 bf16x3, "context" -> -1 (the context's pileup_precision)"""
        if precision is None:
            return None
        if isinstance(precision, str):
            if precision == "context":
                return -1
        elif not isinstance(precision, bool):
            try:
                if operator.index(precision) in (0, 1, 2):
                    return operator.index(precision)
            except TypeError:                                # (a float, a list, an array: no arithmetic either)
                pass
        raise NanoSNPError(f'precision: None, 0 (fp32), 1 (f16x3), 2 (bf16x3) or "context", not {precision!r}')

    def pileup_forward_logits(self, counts, center_idx=None, logits=None, stream=None, precision=None):
        """all four heads as raw logits, fp32 [N,90] (rows 0-20 gt, 21-23 zy, 24-56 indel1, 57-89 indel2); center_idx None: counts is [N,33,18].
        precision: see eval_precision_arg (None: nsnp_pileup_forward_logits, else nsnp_pileup_forward_logits2 in that arithmetic)"""
        import torch
        n = self._eval_inputs(counts, center_idx, "forward_logits")
        logits = logits if logits is not None else torch.empty((n, self.LABEL_WIDTH), dtype=torch.float32, device=counts.device)
        if logits.dtype != torch.float32 or logits.numel() < n * self.LABEL_WIDTH or not logits.is_cuda or not logits.is_contiguous():
            raise NanoSNPError("forward_logits: logits fp32 [N,90] on the device")
        prec = self.eval_precision_arg(precision)
        if prec is None:
            check(self.lib.nsnp_pileup_forward_logits(self.handle, _dptr(counts), _dptr(center_idx), n, _dptr(logits), _stream_ptr(stream)),
                  self.handle, "nsnp_pileup_forward_logits")
        else:
            check(self.lib.nsnp_pileup_forward_logits2(self.handle, _dptr(counts), _dptr(center_idx), n, prec, _dptr(logits), _stream_ptr(stream)),
                  self.handle, "nsnp_pileup_forward_logits2")
        return logits

    @staticmethod
    def pileup_stage_shape(stage, n):
        """name or number of a stage of nsnp_pileup_forward_stage (include/nanosnp.h) -> (number, shape of its image for n sites)"""
        table = {"h0": (0, (n, 33, 128)), "h1c": (1, (n, 128))}
        if isinstance(stage, str):
            if stage not in table:
                raise NanoSNPError(f"pileup_forward_stage: unknown stage {stage!r}")
            return table[stage]
        for num, shape in table.values():
            if not isinstance(stage, bool) and num == operator.index(stage):
                return num, shape
        raise NanoSNPError(f"pileup_forward_stage: unknown stage {stage!r}")

    def pileup_forward_stage(self, counts, stage, center_idx=None, precision="context", stream=None):
        """Test tap: the layer launches of the forward in arithmetic `precision` (0, 1, 2 or "context") under the current options, then
        the image `stage` ("h0": layer 0's h [N,33,128], "h1c": layer 1's h at position 16 [N,128]; or its number) as a plain float32
        tensor, feature = dir * 64 + unit.  One pass: 0 < N <= the reserved chunk."""
        import torch
        n = self._eval_inputs(counts, center_idx, "forward_stage")
        prec = self.eval_precision_arg(precision)
        if prec is None:
            raise NanoSNPError('pileup_forward_stage: precision 0, 1, 2 or "context"')
        num, shape = self.pileup_stage_shape(stage, n)
        out = torch.empty(shape, dtype=torch.float32, device=counts.device)
        check(self.lib.nsnp_pileup_forward_stage(self.handle, _dptr(counts), _dptr(center_idx), n, prec, num, _dptr(out), out.numel(),
                                                 _stream_ptr(stream)), self.handle, "nsnp_pileup_forward_stage")
        return out

    def pileup_eval_windows(self, counts, center_idx, cls, counters, n=None, site_loss=None, pred=None, want_logits=False, stream=None,
                            precision=None):
        """forward + label-smoothed loss + argmax + confusion counts -> (site_loss fp32 [n,4], pred uint8 [n,4], logits fp32 [n,90] or None).
        cls: device uint8 [>= n, 4]; counters: device int64 [EVAL_COUNTERS], added to; n: the sites to run (default: all of center_idx / counts).
        precision: see eval_precision_arg (None: nsnp_pileup_eval_windows, else nsnp_pileup_eval_windows2 in that arithmetic)"""
        import torch
        prec = self.eval_precision_arg(precision)
        n_all = self._eval_inputs(counts, center_idx, "eval_windows")
        n = n_all if n is None else int(n)
        dev = counts.device
        if n < 0 or n > n_all or cls.dtype != torch.uint8 or cls.numel() < 4 * n or not cls.is_cuda or not cls.is_contiguous():
            raise NanoSNPError("eval_windows: cls uint8 [N,4] on the device, one row per site")
        if counters.dtype != torch.int64 or counters.numel() != self.EVAL_COUNTERS or not counters.is_cuda or not counters.is_contiguous():
            raise NanoSNPError(f"eval_windows: counters int64 [{self.EVAL_COUNTERS}] on the device")
        site_loss = site_loss if site_loss is not None else torch.empty((n, 4), dtype=torch.float32, device=dev)
        pred = pred if pred is not None else torch.empty((n, 4), dtype=torch.uint8, device=dev)
        if (site_loss.dtype != torch.float32 or site_loss.numel() < 4 * n or not site_loss.is_cuda or not site_loss.is_contiguous()
                or pred.dtype != torch.uint8 or pred.numel() < 4 * n or not pred.is_cuda or not pred.is_contiguous()):
            raise NanoSNPError("eval_windows: site_loss fp32 [N,4] and pred uint8 [N,4] on the device")
        logits = torch.empty((n, self.LABEL_WIDTH), dtype=torch.float32, device=dev) if want_logits else None
        if prec is None:
            check(self.lib.nsnp_pileup_eval_windows(self.handle, _dptr(counts), _dptr(center_idx), _dptr(cls), n, _dptr(site_loss), _dptr(pred),
                                                    _dptr(counters), _dptr(logits), _stream_ptr(stream)), self.handle, "nsnp_pileup_eval_windows")
        else:
            check(self.lib.nsnp_pileup_eval_windows2(self.handle, _dptr(counts), _dptr(center_idx), _dptr(cls), n, prec, _dptr(site_loss),
                                                     _dptr(pred), _dptr(counters), _dptr(logits), _stream_ptr(stream)),
                  self.handle, "nsnp_pileup_eval_windows2")
        return site_loss, pred, logits

    def pileup_batch_loss(self, site_loss, batch_size, n=None, stream=None):
        """float64 sums of site_loss fp32 [n,4] per batch of batch_size rows -> device float64 [ceil(n / batch_size), 4]"""
        import torch
        if site_loss.dtype != torch.float32 or not site_loss.is_cuda or not site_loss.is_contiguous():
            raise NanoSNPError("batch_loss: site_loss fp32 [N,4] on the device")
        n = int(site_loss.numel() // 4) if n is None else int(n)
        if int(batch_size) < 1 or n < 0 or 4 * n > site_loss.numel():
            raise NanoSNPError("batch_loss: batch_size >= 1 and n rows within site_loss")
        nb = -(-n // int(batch_size))
        out = torch.empty((nb, 4), dtype=torch.float64, device=site_loss.device)
        check(self.lib.nsnp_pileup_batch_loss(self.handle, _dptr(site_loss), n, int(batch_size), _dptr(out), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_batch_loss")
        return out

    # ---- training (include/nanosnp.h; fp32 only) ----
    TRAIN_SHAPES = ([(256, 18), (256, 64), (256,), (256,)] * 2 + [(256, 128), (256, 64), (256,), (256,)] * 2 +
                    [(128, 128), (128,), (256, 128), (256,), (21, 256), (21,), (3, 256), (3,)])        # the 24 tensors of pileup_load_weights

    def pileup_train_reserve(self, max_sites):
        """workspace of pileup_loss_grad for chunks of max_sites sites (about 194 KB per site); synchronous"""
        check(self.lib.nsnp_pileup_train_reserve(self.handle, int(max_sites)), self.handle, "nsnp_pileup_train_reserve")

    def _train_tensors(self, tensors, what):
        import torch
        if len(tensors) != 24:
            raise NanoSNPError(f"loss_grad: expected 24 {what}, got {len(tensors)}")
        for t, shape in zip(tensors, self.TRAIN_SHAPES):
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise NanoSNPError(f"loss_grad: {what} must be contiguous device fp32 tensors in state-dict shapes, got {tuple(t.shape)} for {shape}")
        return (C.c_void_p * 24)(*[t.data_ptr() for t in tensors])

    def pileup_loss_grad(self, params, counts, center_idx, cls, grads, keep_mask=None, keep_scale=1.0, n=None, site_loss=None, pred=None,
                         stream=None):
        """forward, label-smoothed loss and backward of a batch: grads (24 device fp32 tensors in the shapes of params) are OVERWRITTEN with
        d(mean gt + mean zy) / d(param) -> (site_loss fp32 [n,2], pred uint8 [n,2]).  params: the 24 device tensors in state-dict order;
        cls: device uint8 [>= n, 4]; keep_mask: None or device uint8 [n,33,128], layer 1 sees h0 * keep_mask * keep_scale; n: the sites to
        run (default: all of center_idx / counts).  Needs pileup_train_reserve; a larger batch runs in chunks of the reservation."""
        import torch
        n_all = self._eval_inputs(counts, center_idx, "loss_grad")
        n = n_all if n is None else int(n)
        dev = counts.device
        if n < 0 or n > n_all or cls.dtype != torch.uint8 or cls.numel() < 4 * n or not cls.is_cuda or not cls.is_contiguous():
            raise NanoSNPError("loss_grad: cls uint8 [N,4] on the device, one row per site")
        pp, gp = self._train_tensors(params, "parameters"), self._train_tensors(grads, "gradients")
        if keep_mask is not None and (keep_mask.dtype != torch.uint8 or not keep_mask.is_cuda or not keep_mask.is_contiguous()
                                      or keep_mask.numel() < n * 33 * 128 or (keep_mask.dim() == 3 and tuple(keep_mask.shape[1:]) != (33, 128))):
            raise NanoSNPError("loss_grad: keep_mask uint8 [N,33,128] on the device")
        site_loss = site_loss if site_loss is not None else torch.empty((n, 2), dtype=torch.float32, device=dev)
        pred = pred if pred is not None else torch.empty((n, 2), dtype=torch.uint8, device=dev)
        if (site_loss.dtype != torch.float32 or site_loss.numel() < 2 * n or not site_loss.is_cuda or not site_loss.is_contiguous()
                or pred.dtype != torch.uint8 or pred.numel() < 2 * n or not pred.is_cuda or not pred.is_contiguous()):
            raise NanoSNPError("loss_grad: site_loss fp32 [N,2] and pred uint8 [N,2] on the device")
        check(self.lib.nsnp_pileup_loss_grad(self.handle, pp, _dptr(counts), _dptr(center_idx), _dptr(cls), n, _dptr(keep_mask),
                                             float(keep_scale), gp, _dptr(site_loss), _dptr(pred), _stream_ptr(stream)),
              self.handle, "nsnp_pileup_loss_grad")
        return site_loss, pred

    @staticmethod
    def hap_train_shapes(n_features=105, n_gt=10, n_zy=3):
        """the shapes of the 58 tensors of haplotype_model.state_dict_keys() at these dims (hidden size 256, three layers)"""
        enc = []
        for l in range(3):
            enc += [(1024, n_features if l == 0 else 512), (1024, 256), (1024,), (1024,)] * 2
        enc += [(256, 512), (256,)]
        return enc + enc + [(256, 512), (256,), (n_gt, 256), (n_gt,), (n_zy, 256), (n_zy,)]

    def hap_train_reserve(self, max_sites, n_features=105, n_gt=10, n_zy=3):
        """workspace of hap_loss_grad for chunks of max_sites sites of a model of these dims (1,652,864 bytes per site); synchronous"""
        check(self.lib.nsnp_hap_train_reserve(self.handle, int(max_sites), int(n_features), int(n_gt), int(n_zy)), self.handle,
              "nsnp_hap_train_reserve")
        self._hap_train_dims = (int(n_features), int(n_gt), int(n_zy))

    def _hap_train_tensors(self, tensors, shapes, what):
        import torch
        if len(tensors) != 58:
            raise NanoSNPError(f"hap_loss_grad: expected 58 {what}, got {len(tensors)}")
        for t, shape in zip(tensors, shapes):
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != shape:
                raise NanoSNPError(f"hap_loss_grad: {what} must be contiguous device fp32 tensors in the state-dict shapes of the reserved dims, "
                                   f"got {tuple(t.shape)} for {shape}")
        return (C.c_void_p * 58)(*[t.data_ptr() for t in tensors])

    def hap_loss_grad(self, params, xp, xh, cls, grads, keep_masks=None, keep_scale=1.0, n=None, site_loss=None, pred=None, stream=None):
        """forward, label-smoothed loss and backward of a batch of the HaplotypeModel: grads (58 device fp32 tensors in the shapes of params)
        are OVERWRITTEN with d(mean gt + mean zy) / d(param) -> (site_loss fp32 [n,2], pred uint8 [n,2]).  params: the 58 device tensors in
        state-dict order; xp [N,F,33], xh [N,F,11] contiguous device fp32; cls: device uint8 [>= n, 2]; keep_masks: None or four device uint8
        tensors [n,33,512], [n,33,512], [n,11,512], [n,11,512] (behind pileup layers 0 and 1, haplotype layers 0 and 1), the next layer sees
        h * mask * keep_scale; n: the sites to run (default: all of xp).  Needs hap_train_reserve with the dims of these tensors; a larger
        batch runs in chunks of the reservation."""
        import torch
        dims = getattr(self, "_hap_train_dims", None)
        if dims is None:
            raise NanoSNPError("hap_loss_grad: hap_train_reserve first")
        F, n_gt, n_zy = dims
        for t, l, what in ((xp, 33, "xp"), (xh, 11, "xh")):
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[2] != l:
                raise NanoSNPError(f"hap_loss_grad: {what} must be a contiguous device fp32 [N,F,{l}]")
            if t.shape[1] != F:
                raise NanoSNPError(f"hap_loss_grad: {what} has {t.shape[1]} features, the reservation is for {F}")
        n_all = int(xp.shape[0])
        n = n_all if n is None else int(n)
        dev = xp.device
        if n < 0 or n > n_all or xh.shape[0] < n:
            raise NanoSNPError("hap_loss_grad: n sites within xp and xh")
        if cls.dtype != torch.uint8 or cls.numel() < 2 * n or not cls.is_cuda or not cls.is_contiguous():
            raise NanoSNPError("hap_loss_grad: cls uint8 [N,2] on the device, one row per site")
        shapes = self.hap_train_shapes(F, n_gt, n_zy)
        pp, gp = self._hap_train_tensors(params, shapes, "parameters"), self._hap_train_tensors(grads, shapes, "gradients")
        mp = None
        if keep_masks is not None:
            if len(keep_masks) != 4:
                raise NanoSNPError("hap_loss_grad: four keep masks (pileup layers 0 and 1, haplotype layers 0 and 1)")
            for m, l in zip(keep_masks, (33, 33, 11, 11)):
                if (m.dtype != torch.uint8 or not m.is_cuda or not m.is_contiguous() or m.dim() != 3 or m.shape[0] < n
                        or tuple(m.shape[1:]) != (l, 512)):
                    raise NanoSNPError(f"hap_loss_grad: keep mask uint8 [N,{l},512] on the device")
            mp = (C.c_void_p * 4)(*[m.data_ptr() for m in keep_masks])
        site_loss = site_loss if site_loss is not None else torch.empty((n, 2), dtype=torch.float32, device=dev)
        pred = pred if pred is not None else torch.empty((n, 2), dtype=torch.uint8, device=dev)
        if (site_loss.dtype != torch.float32 or site_loss.numel() < 2 * n or not site_loss.is_cuda or not site_loss.is_contiguous()
                or pred.dtype != torch.uint8 or pred.numel() < 2 * n or not pred.is_cuda or not pred.is_contiguous()):
            raise NanoSNPError("hap_loss_grad: site_loss fp32 [N,2] and pred uint8 [N,2] on the device")
        check(self.lib.nsnp_hap_loss_grad(self.handle, pp, _dptr(xp), _dptr(xh), _dptr(cls), n, mp, float(keep_scale), gp, _dptr(site_loss),
                                          _dptr(pred), _stream_ptr(stream)), self.handle, "nsnp_hap_loss_grad")
        return site_loss, pred

    def optim_scratch_floats(self, counts):
        """floats of the partial-sum scratch of optim_step for tensors of these element counts"""
        arr = (C.c_int64 * len(counts))(*[int(c) for c in counts])
        n = int(self.lib.nsnp_optim_scratch_floats(len(counts), arr))
        if n < 1:
            raise NanoSNPError(f"optim_step: 1..{OPTIM_MAX_TENSORS} tensors of at least one element each")
        return n

    def optim_tensors(self, params, grads, exp_avg, exp_avg_sq, slow=None):
        """the tensor lists of optim_step, checked once -> OptimTensors.  Every list: as many contiguous fp32 tensors on this context's device
        as params, entry i in the shape of params[i]; views into a larger buffer are fine.  slow None: no Lookahead buffers (sync 0 only).
        exp_avg / exp_avg_sq are the two state tables of optim_kind_step as well, either None where its kind has no such state."""
        import torch
        n = len(params)
        if not 1 <= n <= OPTIM_MAX_TENSORS:
            raise NanoSNPError(f"optim_step: 1..{OPTIM_MAX_TENSORS} tensors, got {n}")
        lists = {"params": params, "grads": grads}
        for what, ts in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("slow", slow)):
            if ts is not None:
                lists[what] = ts
        for what, ts in lists.items():
            if len(ts) != n:
                raise NanoSNPError(f"optim_step: {len(ts)} {what} for {n} params")
            for t, p in zip(ts, params):
                if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device.index != self.device
                        or not t.is_contiguous() or t.shape != p.shape or t.numel() < 1):
                    raise NanoSNPError(f"optim_step: {what} must be non-empty contiguous fp32 tensors on cuda:{self.device} in the shapes of params")
        ot = OptimTensors()
        ot.n, ot.keep, ot.device = n, lists, params[0].device
        for what in ("params", "grads", "exp_avg", "exp_avg_sq", "slow"):
            setattr(ot, what, (C.c_void_p * n)(*[t.data_ptr() for t in lists[what]]) if what in lists else None)
        ot.grad_ptrs = tuple(t.data_ptr() for t in grads)
        ot.counts = (C.c_int64 * n)(*[t.numel() for t in params])
        ot.scratch_floats = self.optim_scratch_floats([t.numel() for t in params])
        return ot

    def optim_step(self, tensors, args, scratch=None, grad_norm_out=None, stream=None):
        """One fused optimiser step (nsnp_optim_step: gradient norm, clip, Adam / RAdam moments and update, Lookahead sync; two launches,
        asynchronous).  tensors: an OptimTensors, or the tuple (params, grads, exp_avg, exp_avg_sq[, slow]) to check now; args: an OptimArgs
        (the float64 scalars of this step); scratch: device fp32 of at least tensors.scratch_floats, made here when None and needed;
        grad_norm_out: None or one device fp32 that receives the unclipped norm.  -> grad_norm_out."""
        import torch
        ot = tensors if isinstance(tensors, OptimTensors) else self.optim_tensors(*tensors)
        if not isinstance(args, OptimArgs):
            raise NanoSNPError("optim_step: args must be an OptimArgs")
        if ot.exp_avg is None or ot.exp_avg_sq is None:
            raise NanoSNPError("optim_step: exp_avg and exp_avg_sq are both needed")
        if args.sync != 0 and ot.slow is None:
            raise NanoSNPError("optim_step: a Lookahead sync needs the slow buffers")
        if scratch is None and (args.max_norm > 0 or grad_norm_out is not None):
            scratch = torch.empty(ot.scratch_floats, dtype=torch.float32, device=ot.device)
        if scratch is not None and (scratch.dtype != torch.float32 or not scratch.is_cuda or scratch.device != ot.device
                                    or not scratch.is_contiguous() or scratch.numel() < ot.scratch_floats):
            raise NanoSNPError(f"optim_step: scratch fp32 [{ot.scratch_floats}] on the device")
        if grad_norm_out is not None and (grad_norm_out.dtype != torch.float32 or not grad_norm_out.is_cuda or grad_norm_out.device != ot.device
                                          or grad_norm_out.numel() != 1):
            raise NanoSNPError("optim_step: grad_norm_out one fp32 on the device")
        check(self.lib.nsnp_optim_step(self.handle, ot.n, ot.params, ot.grads, ot.exp_avg, ot.exp_avg_sq, ot.slow, ot.counts, C.byref(args),
                                       _dptr(scratch), _dptr(grad_norm_out), _stream_ptr(stream)), self.handle, "nsnp_optim_step")
        return grad_norm_out

    def optim_kind_step(self, tensors, args, layer_in=None, layer_out=None, scratch=None, grad_norm_out=None, stream=None):
        """One fused Novograd / SGD / Adadelta step (nsnp_optim_step_kind; two launches, asynchronous).  tensors: an OptimTensors whose
        exp_avg / exp_avg_sq tables are the kind's state_a / state_b (None where the kind has none), or the tuple to check now; args: an
        OptimKindArgs; layer_in / layer_out: Novograd's per-tensor second moments, two different device fp32 [n] (read / written);
        scratch and grad_norm_out as for optim_step.  -> grad_norm_out."""
        import torch
        ot = tensors if isinstance(tensors, OptimTensors) else self.optim_tensors(*tensors)
        if not isinstance(args, OptimKindArgs):
            raise NanoSNPError("optim_kind_step: args must be an OptimKindArgs")
        novo = args.kind == OPTIM_NOVOGRAD
        need_a = args.kind != OPTIM_SGD or args.momentum != 0
        if (need_a and ot.exp_avg is None) or (args.kind == OPTIM_ADADELTA and ot.exp_avg_sq is None):
            raise NanoSNPError("optim_kind_step: a state table of this kind is missing")
        if args.sync != 0 and ot.slow is None:
            raise NanoSNPError("optim_kind_step: a Lookahead sync needs the slow buffers")
        if scratch is None and (novo or args.max_norm > 0 or grad_norm_out is not None):
            scratch = torch.empty(ot.scratch_floats, dtype=torch.float32, device=ot.device)
        if scratch is not None and (scratch.dtype != torch.float32 or not scratch.is_cuda or scratch.device != ot.device
                                    or not scratch.is_contiguous() or scratch.numel() < ot.scratch_floats):
            raise NanoSNPError(f"optim_kind_step: scratch fp32 [{ot.scratch_floats}] on the device")
        if grad_norm_out is not None and (grad_norm_out.dtype != torch.float32 or not grad_norm_out.is_cuda or grad_norm_out.device != ot.device
                                          or grad_norm_out.numel() != 1):
            raise NanoSNPError("optim_kind_step: grad_norm_out one fp32 on the device")
        for t in (layer_in, layer_out):
            if (t is None and novo) or (t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.device != ot.device
                                                           or not t.is_contiguous() or t.numel() < ot.n)):
                raise NanoSNPError(f"optim_kind_step: layer_in / layer_out fp32 [{ot.n}] on the device")
        check(self.lib.nsnp_optim_step_kind(self.handle, ot.n, ot.params, ot.grads, ot.exp_avg, ot.exp_avg_sq, ot.slow, ot.counts, C.byref(args),
                                            _dptr(layer_in), _dptr(layer_out), _dptr(scratch), _dptr(grad_norm_out), _stream_ptr(stream)),
              self.handle, "nsnp_optim_step_kind")
        return grad_norm_out

    def pileup_gather_windows(self, counts, center_idx, stream=None):
        import torch
        n = center_idx.shape[0]
        x = torch.empty((n, 33, 18), dtype=torch.int32, device=counts.device)
        check(self.lib.nsnp_pileup_gather_windows(self.handle, _dptr(counts), _dptr(center_idx), n, _dptr(x),
                                                  _stream_ptr(stream)),
              self.handle, "nsnp_pileup_gather_windows")
        return x

    # ---- HaplotypeModel ----------------------------------------------------------------------
    def hap_features(self, seq, bq, mq, hap, ref_row, stream=None):
        """int32 planes (the reference's bins) or int8 planes (nsnp_hap_features_i8: a quarter of the bytes); ref_row int32"""
        import torch
        n, d, l = seq.shape
        out = torch.empty((n, 105, l), dtype=torch.float32, device=seq.device)
        if seq.dtype == torch.int8:
            if not (bq.dtype == mq.dtype == hap.dtype == torch.int8):
                raise NanoSNPError("hap_features: the four read planes must share one dtype (int32 or int8)")
            if ref_row.dtype != torch.int32:
                raise NanoSNPError("hap_features: ref_row must be int32")
            check(self.lib.nsnp_hap_features_i8(self.handle, _dptr(seq), _dptr(bq), _dptr(mq), _dptr(hap), _dptr(ref_row),
                                                n, d, l, _dptr(out), _stream_ptr(stream)),
                  self.handle, "nsnp_hap_features_i8")
            return out
        check(self.lib.nsnp_hap_features(self.handle, _dptr(seq), _dptr(bq), _dptr(mq), _dptr(hap), _dptr(ref_row),
                                         n, d, l, _dptr(out), _stream_ptr(stream)),
              self.handle, "nsnp_hap_features")
        return out

    TIE_ORDERS = {"stable": 0, "numpy1": 1}       # NSNP_TIE_STABLE, NSNP_TIE_NUMPY1

    def hap_arrange_reads(self, seq, bq, mq, hap, d_out, n_reads=None, stream=None, tie_order="stable"):
        """tie_order: "stable" (ties keep their input order) or "numpy1" (NumPy 1.x argsort(kind="quicksort"), the reference's
        environment: with the rows in the order the reference first sees the reads, the planes equal its bins row for row)"""
        import torch
        if tie_order not in self.TIE_ORDERS:
            raise NanoSNPError(f"hap_arrange_reads: tie_order must be one of {sorted(self.TIE_ORDERS)}, not {tie_order!r}")
        n, r, l = seq.shape
        outs = [torch.empty((n, d_out, l), dtype=torch.int32, device=seq.device) for _ in range(4)]
        depth = torch.empty(n, dtype=torch.int32, device=seq.device)
        check(self.lib.nsnp_hap_arrange_reads2(self.handle, _dptr(seq), _dptr(bq), _dptr(mq), _dptr(hap), _dptr(n_reads),
                                               n, r, l, int(d_out), self.TIE_ORDERS[tie_order], *[_dptr(o) for o in outs],
                                               _dptr(depth), _stream_ptr(stream)),
              self.handle, "nsnp_hap_arrange_reads2")
        return outs[0], outs[1], outs[2], outs[3], depth

    # ---- stage-4 read matrices from alignment records (hap_reads.hip) ----
    def _read_scratch(self, rec, cols):
        import torch
        need = self.lib.nsnp_hap_read_scratch_bytes(rec.n, cols.shape[0])
        if need == 0:
            raise NanoSNPError("hap_read_*: more than 2^31 - 16 records or columns")
        return torch.empty(need, dtype=torch.uint8, device=cols.device)

    @staticmethod
    def _read_cols(rec, cols):
        import torch
        if cols.dtype != torch.int64 or cols.dim() != 1 or not cols.is_contiguous() or cols.device != rec.start.device:
            raise NanoSNPError("hap_read_*: cols must be a contiguous int64 vector on the records' device")

    def hap_read_depths(self, rec, cols, want_rows=False, stream=None):
        """rec: readmatrix.AlignmentRecords.to_device(); cols: int64 cuda [P], strictly increasing 1-based positions.
        -> depth int32 [P] (records whose reference span holds the column), with want_rows also int64 [1]: the records that cover
        at least one column."""
        import torch
        self._read_cols(rec, cols)
        P = cols.shape[0]
        depth = torch.empty(P, dtype=torch.int32, device=cols.device)
        rows = torch.empty(1, dtype=torch.int64, device=cols.device) if want_rows else None
        scratch = self._read_scratch(rec, cols)
        check(self.lib.nsnp_hap_read_depths(self.handle, _dptr(rec.start), _dptr(rec.cigar), _dptr(rec.cigar_off), rec.n, _dptr(cols), P,
                                            _dptr(depth), _dptr(rows), _dptr(scratch), _stream_ptr(stream)),
              self.handle, "nsnp_hap_read_depths")
        scratch.record_stream(stream if stream is not None else torch.cuda.current_stream())
        return (depth, rows) if want_rows else depth

    def hap_read_matrices(self, rec, cols, max_coverage, cap_rows, stream=None):
        """-> (seq, hap, baseq, mapq) int32 cuda [cap_rows, P], row_record int64 [cap_rows], meta int64 [4] = {rows, status, record,
        column} (include/nanosnp.h).  cap_rows must be at least the row count (hap_read_depths(..., want_rows=True)); the first
        `rows` rows are written, each cell once."""
        import torch
        self._read_cols(rec, cols)
        P, cap = cols.shape[0], int(cap_rows)
        dev = cols.device
        outs = [torch.empty((cap, P), dtype=torch.int32, device=dev) for _ in range(4)]
        row_record = torch.empty(cap, dtype=torch.int64, device=dev)
        meta = torch.empty(4, dtype=torch.int64, device=dev)
        scratch = self._read_scratch(rec, cols)
        check(self.lib.nsnp_hap_read_matrices(self.handle, _dptr(rec.start), _dptr(rec.mapq), _dptr(rec.hp), _dptr(rec.cigar),
                                              _dptr(rec.cigar_off), _dptr(rec.seq), _dptr(rec.qual), _dptr(rec.seq_off), rec.n, _dptr(cols),
                                              P, min(max(int(max_coverage), -1), 2 ** 31 - 1), *[_dptr(o) for o in outs], cap, _dptr(row_record), _dptr(meta),
                                              _dptr(scratch), _stream_ptr(stream)),
              self.handle, "nsnp_hap_read_matrices")
        scratch.record_stream(stream if stream is not None else torch.cuda.current_stream())
        return outs[0], outs[1], outs[2], outs[3], row_record, meta

    # ---- stage-4 site groups from the call rows (pileup_groups.hip) ----
    GROUPS_WRITTEN, GROUPS_DICT, GROUPS_CANDIDATE, GROUPS_SUPPORT, GROUPS_GROUP = 1, 2, 4, 8, 16
    GROUPS_KEY_ORDER = 1

    def pileup_select_groups(self, rows, ref_base, run_off, cuts, adjacent_size=5, batch_size=1000, cap_groups=None, meta=None, stream=None):
        """rows: float64 cuda [N,13] (pileup_call_rows); ref_base: uint8 cuda [N]; run_off: int64 cuda [n_runs + 1], the rows of every
        contig; cuts: float32 cuda [8] (merge.group_cuts).  -> group_rows int32 [cap, 2A+1], group_keys int64 [cap, 2A+1], meta int64 [4] =
        {groups found, status, first offending row, supports} (include/nanosnp.h; `meta` may be a pinned tensor), flags uint8 [N] (the
        flag byte of every row: GROUPS_WRITTEN | _DICT | _CANDIDATE | _SUPPORT | _GROUP).  cap_groups None: one group per row, the most
        there can be.  Nothing comes back through the host: slice the outputs with meta[0] once the stream has passed the call."""
        import torch
        if (rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] != 13 or not rows.is_cuda or not rows.is_contiguous()):
            raise NanoSNPError("pileup_select_groups: rows must be a contiguous float64 cuda tensor [N,13]")
        n, dev = int(rows.shape[0]), rows.device
        for name, t, dt, ok in (("ref_base", ref_base, torch.uint8, ref_base.numel() == n), ("run_off", run_off, torch.int64, run_off.numel() >= 1),
                                ("cuts", cuts, torch.float32, cuts.numel() == 8)):
            if t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.device != dev or not ok:
                raise NanoSNPError(f"pileup_select_groups: {name} must be a contiguous {dt} vector on the rows' device (ref_base [N], run_off "
                                   "[n_runs + 1], cuts [8])")
        a, cap = int(adjacent_size), n if cap_groups is None else int(cap_groups)
        need = self.lib.nsnp_pileup_groups_scratch_bytes(n)
        if need == 0:
            raise NanoSNPError("pileup_select_groups: more than 2^31 - 16 rows")
        w = 2 * a + 1 if 1 <= a <= 32 else 1
        group_rows = torch.empty((max(cap, 0), w), dtype=torch.int32, device=dev)
        group_keys = torch.empty((max(cap, 0), w), dtype=torch.int64, device=dev)
        if meta is None:
            meta = torch.empty(4, dtype=torch.int64, device=dev)
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        check(self.lib.nsnp_pileup_select_groups(self.handle, _dptr(rows), _dptr(ref_base), n, _dptr(run_off), int(run_off.numel()) - 1, int(batch_size),
                                                 a, _dptr(cuts), _dptr(group_rows), _dptr(group_keys), cap, _dptr(meta), _dptr(scratch),
                                                 _stream_ptr(stream)),
              self.handle, "nsnp_pileup_select_groups")
        scratch.record_stream(stream if stream is not None else torch.cuda.current_stream())
        return group_rows, group_keys, meta, scratch[:n]

    def hap_load_weights(self, tensors, n_features=105, hidden=256, n_layers=3, n_gt=10, n_zy=3):
        import numpy as np
        arrs = [np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
                for t in tensors]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        check(self.lib.nsnp_hap_load_weights(self.handle, ptrs, len(arrs), n_features, hidden, n_layers, n_gt, n_zy),
              self.handle, "nsnp_hap_load_weights")
        self._hap_dims = (n_gt, n_zy)

    # ---- legacy CatModel (HaplotypeModel/predict.py -> model.CatModel) ----
    def cat_load_weights(self, tensors):
        """tensors: the 132 floating-point tensors of CatModel.state_dict() in order (num_batches_tracked skipped)."""
        import numpy as np
        arrs = [np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float32)
                for t in tensors]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        check(self.lib.nsnp_cat_load_weights(self.handle, ptrs, len(arrs)), self.handle, "nsnp_cat_load_weights")

    def cat_forward(self, g0, g1, stream=None):
        """g0, g1: float32 cuda [N,40,11,5] -> softmax probabilities [N,10] (model.py:332-358)."""
        import torch
        if tuple(g0.shape[1:]) != (40, 11, 5) or g0.shape != g1.shape:
            raise NanoSNPError(f"cat_forward: g0/g1 must be [N,40,11,5], got {tuple(g0.shape)} / {tuple(g1.shape)}")
        g0 = g0.contiguous().float(); g1 = g1.contiguous().float()
        n = g0.shape[0]
        gt = torch.empty((n, 10), dtype=torch.float32, device=g0.device)
        check(self.lib.nsnp_cat_forward(self.handle, _dptr(g0), _dptr(g1), n, _dptr(gt), _stream_ptr(stream)),
              self.handle, "nsnp_cat_forward")
        return gt

    @staticmethod
    def cat_stage_shape(stage, n):
        """name or number of a stage of nsnp_cat_forward_stage (include/nanosnp.h) -> (number, shape of its image for n sites)"""
        ch, hs = (32, 64, 128, 128, 256, 256), (40, 20, 10, 10, 3, 3)
        table = {"pixels": (0, (n, 10, 40, 11)), "seq0": (16, (11, n, 256)), "pct_features": (17, (11, n, 20)),
                 "pct_h0": (18, (11, n, 512)), "pct_h1": (19, (11, n, 512)), "pct_h2": (20, (6, n, 512)), "pct_linear": (21, (n, 256)),
                 "rnn0_h": (22, (11, n, 512)), "rnn0_emb": (23, (11, n, 256)), "rnn1_h": (24, (6, n, 512)), "cat": (25, (n, 512)),
                 "pool0": (13, (n, 32, 20, 11)), "pool1": (14, (n, 64, 10, 11)), "pool3": (15, (n, 128, 3, 11))}
        for i in range(6):
            table[f"block{i}_y"] = (1 + 2 * i, (n, ch[i], hs[i], 11)); table[f"block{i}_out"] = (2 + 2 * i, (n, ch[i], hs[i], 11))
        if isinstance(stage, str):
            if stage not in table:
                raise NanoSNPError(f"cat_forward_stage: unknown stage {stage!r}")
            return table[stage]
        for num, shape in table.values():
            if num == int(stage):
                return num, shape
        raise NanoSNPError(f"cat_forward_stage: unknown stage {stage!r}")

    def cat_forward_stage(self, g0, g1, stage, stream=None):
        """Test tap: the launches of cat_forward up to and including `stage` (a name of cat_stage_shape or its number), then that
        stage's image as a plain float32 tensor in natural order.  One pass: 0 < N <= 4096."""
        import torch
        if tuple(g0.shape[1:]) != (40, 11, 5) or g0.shape != g1.shape:
            raise NanoSNPError(f"cat_forward_stage: g0/g1 must be [N,40,11,5], got {tuple(g0.shape)} / {tuple(g1.shape)}")
        g0 = g0.contiguous().float(); g1 = g1.contiguous().float()
        n = g0.shape[0]
        num, shape = self.cat_stage_shape(stage, n)
        out = torch.empty(shape, dtype=torch.float32, device=g0.device)
        check(self.lib.nsnp_cat_forward_stage(self.handle, _dptr(g0), _dptr(g1), n, num, _dptr(out), out.numel(), _stream_ptr(stream)),
              self.handle, "nsnp_cat_forward_stage")
        return out

    def cat_groups(self, tag1, tag2, stream=None):
        """tag1 / tag2: (read, baseq, mapq) int32 cuda [N,depth,L] per tag -> [N,40,L,5] float32 (dataset.py:862-915)."""
        import torch
        r1, q1, m1 = [t.contiguous() for t in tag1]
        r2, q2, m2 = [t.contiguous() for t in tag2]
        n, d1, l = r1.shape
        d2 = r2.shape[1]
        g = torch.empty((n, 40, l, 5), dtype=torch.float32, device=r1.device)
        check(self.lib.nsnp_cat_groups(self.handle, _dptr(r1), _dptr(q1), _dptr(m1), d1, _dptr(r2), _dptr(q2), _dptr(m2), d2,
                                       n, l, _dptr(g), _stream_ptr(stream)), self.handle, "nsnp_cat_groups")
        return g

    def hap_forward(self, xp, xh, stream=None):
        import torch
        n = xp.shape[0]
        n_gt, n_zy = self._hap_dims
        gt = torch.empty((n, n_gt), dtype=torch.float32, device=xp.device)
        zy = torch.empty((n, n_zy), dtype=torch.float32, device=xp.device)
        check(self.lib.nsnp_hap_forward(self.handle, _dptr(xp), _dptr(xh), n, _dptr(gt), _dptr(zy),
                                        _stream_ptr(stream)),
              self.handle, "nsnp_hap_forward")
        return gt, zy

    # ---- scoring a HaplotypeModel checkpoint on labelled sites (include/nanosnp.h; every hap_precision) ----
    HAP_EVAL_WAVES_PER_CU = 32                  # NSNP_HAP_EVAL_WAVES_PER_CU: the persistent heads kernel takes one site per wave and trip

    def hap_label_classes(self, label, cls=None, rows=None, meta=None, stream=None):
        """label: device int32 [N,3] = {confident, gt21, zygosity} -> (cls uint8 [N,2], rows int64 [N], meta int64 [4]): the first meta[0]
        rows of cls / rows are the kept rows' classes {gt, max(zy, 0)} and their indices, in order; meta = {kept, unscorable, refcalls kept,
        variants kept}.  meta may be pinned host memory; the count is only known behind the launch."""
        import torch
        if label.dtype != torch.int32 or not label.is_cuda or not label.is_contiguous() or label.dim() != 2 or label.shape[1] != 3:
            raise NanoSNPError("hap_label_classes: label must be a contiguous device int32 [N,3]")
        n, dev = int(label.shape[0]), label.device
        cls = cls if cls is not None else torch.empty((max(n, 1), 2), dtype=torch.uint8, device=dev)
        rows = rows if rows is not None else torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        meta = meta if meta is not None else torch.zeros(4, dtype=torch.int64, device=dev)
        if (cls.dtype != torch.uint8 or cls.numel() < 2 * n or not cls.is_cuda or not cls.is_contiguous() or rows.dtype != torch.int64
                or rows.numel() < n or not rows.is_cuda or not rows.is_contiguous()):
            raise NanoSNPError("hap_label_classes: cls uint8 [N,2] and rows int64 [N] on the device")
        if meta.dtype != torch.int64 or meta.numel() < 4 or not (meta.is_cuda or meta.is_pinned()) or not meta.is_contiguous():
            raise NanoSNPError("hap_label_classes: meta int64 [4] on the device or in pinned memory")
        check(self.lib.nsnp_hap_label_classes(self.handle, _dptr(label), n, _dptr(cls), _dptr(rows), meta.data_ptr(), _stream_ptr(stream)),
              self.handle, "nsnp_hap_label_classes")
        return cls, rows, meta

    HAP_PN_VALUE_MAX = 4194304.0                # NSNP_HAP_PN_VALUE_MAX

    def hap_train_samples(self, cls, kept, pn_value, seed, draw=0, samples=None, meta=None, stream=None):
        """cls: device uint8 [>= kept, 2] as hap_label_classes leaves it -> (samples int64, meta int64 [4]): the training sample list of a pass
        under pn_value upsampling (nsnp_hap_train_samples): the first meta[0] entries of samples are indices in [0, kept) into the kept
        list; meta = {M, refcalls, variants, blocks}, on the device or in pinned memory.  seed: 64 bits, draw: 32 bits (the pass counter).
        samples None: a new tensor with room for any split of `kept` rows; a given one smaller than M is refused with nothing written.
        The entry waits for the stream once (for the two counts)."""
        import torch
        kept, pn_value, seed, draw = int(kept), float(pn_value), int(seed), int(draw)
        if cls.dtype != torch.uint8 or not cls.is_cuda or not cls.is_contiguous() or kept < 0 or cls.numel() < 2 * kept:
            raise NanoSNPError("hap_train_samples: cls must be a contiguous device uint8 [kept,2]")
        if not (0.0 <= pn_value <= self.HAP_PN_VALUE_MAX):
            raise NanoSNPError(f"hap_train_samples: pn_value in [0, {self.HAP_PN_VALUE_MAX:.0f}], got {pn_value}")
        if not (0 <= seed < 1 << 64 and 0 <= draw < 1 << 32):
            raise NanoSNPError("hap_train_samples: seed in [0, 2^64) and draw in [0, 2^32)")
        dev = cls.device
        if samples is None:
            samples = torch.empty(max(kept + -(-kept // 1000) * int(1000.0 * pn_value), 1), dtype=torch.int64, device=dev)
        meta = meta if meta is not None else torch.zeros(4, dtype=torch.int64, device=dev)
        if samples.dtype != torch.int64 or not samples.is_cuda or not samples.is_contiguous():
            raise NanoSNPError("hap_train_samples: samples int64 on the device")
        if meta.dtype != torch.int64 or meta.numel() < 4 or not (meta.is_cuda or meta.is_pinned()) or not meta.is_contiguous():
            raise NanoSNPError("hap_train_samples: meta int64 [4] on the device or in pinned memory")
        check(self.lib.nsnp_hap_train_samples(self.handle, _dptr(cls), kept, pn_value, seed, draw, _dptr(samples), int(samples.numel()),
                                              meta.data_ptr(), _stream_ptr(stream)), self.handle, "nsnp_hap_train_samples")
        return samples, meta

    def hap_eval_counters(self, device=None):
        """a zeroed counter tensor for hap_eval: int64 [n_gt * n_gt + n_zy * n_zy]"""
        import torch
        n_gt, n_zy = self._hap_dims
        return torch.zeros(n_gt * n_gt + n_zy * n_zy, dtype=torch.int64, device=device if device is not None else torch.device("cuda", self.device))

    def hap_eval(self, xp, xh, cls, counters, n=None, site_loss=None, pred=None, want_logits=False, stream=None):
        """forward + label-smoothed loss + argmax + confusion counts -> (site_loss fp32 [n,2], pred uint8 [n,2], logits fp32 [n, n_gt + n_zy] or
        None).  xp [N,F,33], xh [N,F,11] contiguous device fp32; cls: device uint8 [>= n, 2]; counters: device int64 [n_gt^2 + n_zy^2], added
        to; n: the sites to run (default: all of xp)"""
        import torch
        if not hasattr(self, "_hap_dims"):
            raise NanoSNPError("hap_eval: weights not loaded")
        n_gt, n_zy = self._hap_dims
        for t, l, what in ((xp, 33, "xp"), (xh, 11, "xh")):
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.dim() != 3 or t.shape[2] != l:
                raise NanoSNPError(f"hap_eval: {what} must be a contiguous device fp32 [N,F,{l}]")
        n_all = int(xp.shape[0])
        n = n_all if n is None else int(n)
        dev = xp.device
        if n < 0 or n > n_all or xh.shape[0] < n or xh.shape[1] != xp.shape[1]:
            raise NanoSNPError("hap_eval: n sites within xp and xh, which share their feature count")
        if cls.dtype != torch.uint8 or cls.numel() < 2 * n or not cls.is_cuda or not cls.is_contiguous():
            raise NanoSNPError("hap_eval: cls uint8 [N,2] on the device, one row per site")
        if counters.dtype != torch.int64 or counters.numel() != n_gt * n_gt + n_zy * n_zy or not counters.is_cuda or not counters.is_contiguous():
            raise NanoSNPError(f"hap_eval: counters int64 [{n_gt * n_gt + n_zy * n_zy}] on the device")
        site_loss = site_loss if site_loss is not None else torch.empty((n, 2), dtype=torch.float32, device=dev)
        pred = pred if pred is not None else torch.empty((n, 2), dtype=torch.uint8, device=dev)
        if (site_loss.dtype != torch.float32 or site_loss.numel() < 2 * n or not site_loss.is_cuda or not site_loss.is_contiguous()
                or pred.dtype != torch.uint8 or pred.numel() < 2 * n or not pred.is_cuda or not pred.is_contiguous()):
            raise NanoSNPError("hap_eval: site_loss fp32 [N,2] and pred uint8 [N,2] on the device")
        logits = torch.empty((n, n_gt + n_zy), dtype=torch.float32, device=dev) if want_logits else None
        check(self.lib.nsnp_hap_eval(self.handle, _dptr(xp), _dptr(xh), _dptr(cls), n, _dptr(site_loss), _dptr(pred), _dptr(counters),
                                     _dptr(logits), _stream_ptr(stream)), self.handle, "nsnp_hap_eval")
        return site_loss, pred, logits

    def hap_batch_loss(self, site_loss, batch_size, n=None, stream=None):
        """float64 sums of site_loss fp32 [n,2] per batch of batch_size rows -> device float64 [ceil(n / batch_size), 2]"""
        import torch
        if site_loss.dtype != torch.float32 or not site_loss.is_cuda or not site_loss.is_contiguous():
            raise NanoSNPError("hap_batch_loss: site_loss fp32 [N,2] on the device")
        n = int(site_loss.numel() // 2) if n is None else int(n)
        if int(batch_size) < 1 or n < 0 or 2 * n > site_loss.numel():
            raise NanoSNPError("hap_batch_loss: batch_size >= 1 and n rows within site_loss")
        nb = -(-n // int(batch_size))
        out = torch.empty((nb, 2), dtype=torch.float64, device=site_loss.device)
        check(self.lib.nsnp_hap_batch_loss(self.handle, _dptr(site_loss), n, int(batch_size), _dptr(out), _stream_ptr(stream)),
              self.handle, "nsnp_hap_batch_loss")
        return out
