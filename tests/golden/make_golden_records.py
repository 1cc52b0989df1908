#!/usr/bin/env python3
"""Generate tests/golden/hap_records.npz: create_pileup_haplotype.single_group_pileup_haplotype_feature (:22-214) itself on reads
with insertions, soft and hard clips, deletions, reference skips and = / X ops.

    python tests/golden/make_golden_records.py

Development container only (the reference's HaplotypeModel directory under $NANOSNP_REFERENCE, default /root/reference).  The
function iterates tests/record_rules.py's RecordSamfile, the per-base stand-in for a pysam.AlignmentFile, over
synth_records(SEED, "mixed") and tests.helpers.synth_groups(GROUP_SEED): four groups.  Per group the fixture holds the filtered,
HP-sorted matrices the function returns (keys g{g}_{h,p}_out_{seq,bq,mq,hap}, as hap_arrange.npz names them), its position
lists and the two maximum depths.  The records are rebuilt from the seed by the test; a CRC-32 of their arrays is stored so
that another random stream is an error, not a comparison against the wrong reads."""
from __future__ import annotations

import contextlib
import io
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NANOSNP_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SEED, GROUP_SEED = 41, 78


def records_crc(arrays):
    return zlib.crc32(b"".join(np.ascontiguousarray(arrays[k]).tobytes() for k in
                               ("start", "mapq", "hp", "cigar", "cigar_off", "seq", "qual", "seq_off")))


def main():
    import make_golden
    make_golden._stub_modules()
    sys.path.insert(0, os.path.join(REF, "HaplotypeModel"))
    import create_pileup_haplotype as cph        # noqa: E402  (reference module)
    from select_hetesnp_homosnp import SNPItem   # noqa: E402
    from tests import record_rules as rr
    from tests.helpers import synth_groups
    records = rr.synth_records(SEED, "mixed")
    groups = [[SNPItem(c, p, "0/1", 10.0 if k == 5 else 20.0) for k, (c, p) in enumerate(g)] for g in synth_groups(GROUP_SEED)]
    with contextlib.redirect_stdout(io.StringIO()):
        out = cph.single_group_pileup_haplotype_feature(rr.RecordSamfile(records), groups, 10000, 5, 16)
    cand, hpos, hseq, hbq, hmq, hhap, maxh, pseq, pbq, pmq, phap, maxp = out
    assert len(cand) == len(groups) and maxh > 10 and maxp > 10, (len(cand), maxh, maxp)
    fx = {"n_groups": len(groups), "seed": SEED, "group_seed": GROUP_SEED, "records_crc32": records_crc(rr.to_arrays(records))}
    for g in range(len(groups)):
        for tag, outs in (("h", (hseq[g], hbq[g], hmq[g], hhap[g])), ("p", (pseq[g], pbq[g], pmq[g], phap[g]))):
            for nm, o in zip(("seq", "bq", "mq", "hap"), outs):
                fx[f"g{g}_{tag}_out_{nm}"] = np.asarray(o, np.int16)
    fx["candidates"] = np.array(cand)
    fx["haplotype_positions"] = np.array(hpos)
    fx["max_depths"] = np.array([maxh, maxp])
    np.savez_compressed(os.path.join(HERE, "hap_records.npz"), **fx)
    ops = sorted({op for rd in records for op, _ in rd["cigar"]})
    print("hap_records:", len(groups), "groups, depths", [np.asarray(a).shape[0] for a in hseq], [np.asarray(a).shape[0] for a in pseq],
          "ops present", "".join("MIDNSHP=X"[o] for o in ops))


if __name__ == "__main__":
    main()
