"""Stage s1 + s2 of the reference pipeline in one pass on the device:

    <chr>.mpileup text + FASTA  ->  column encode -> candidate windows -> PileupModel -> pileup.vcf

replacing DNA_CreateCanSnpTensor -> DNA_CreatePredictData -> make_bin_predict_data.py ->
PileupModel/predict.py (dna_sv_tensor/src/scripts/make_predict_data.sh:184-234,
scripts/s2_pileup_model_predict.sh:11-16) and the four text/HDF5 files between them.
File reading and VCF writing are host work (native readers / writer in libnanosnp_host.so);
everything between lives in HBM.
"""
from __future__ import annotations

import contextlib
import mmap
import os
from collections import deque, namedtuple

import numpy as np

from . import host
from .predict import COV_CHANNELS


# ---- text ranges -------------------------------------------------------------------------------------------------------------
def _as_bytes_like(text):
    """bytes / bytearray / mmap / numpy uint8 -> (object with find / rfind over the whole text, numpy uint8 view of it)"""
    if isinstance(text, np.ndarray):
        text = memoryview(np.ascontiguousarray(text, np.uint8)).cast("B")
        return bytes(text) if len(text) < (1 << 20) else _MvFind(text), np.frombuffer(text, np.uint8)
    return text, np.frombuffer(text, np.uint8)


class _MvFind:
    """find / rfind of a single byte over a memoryview, through numpy (large numpy inputs only)"""
    def __init__(self, mv):
        self.a = np.frombuffer(mv, np.uint8)

    def __len__(self):
        return int(self.a.size)

    def find(self, ch, lo, hi=None):
        hi = self.a.size if hi is None else hi
        step = 1 << 16
        for s0 in range(lo, hi, step):
            w = np.flatnonzero(self.a[s0:min(hi, s0 + step)] == ch[0])
            if w.size:
                return s0 + int(w[0])
        return -1

    def rfind(self, ch, lo, hi):
        step = 1 << 16
        e = hi
        while e > lo:
            s0 = max(lo, e - step)
            w = np.flatnonzero(self.a[s0:e] == ch[0])
            if w.size:
                return s0 + int(w[-1])
            e = s0
        return -1


@contextlib.contextmanager
def _mapped(path):
    """the bytes of a file, mapped and never copied (b"" for an empty file: nothing to map); unmapped behind the block"""
    with open(path, "rb") as g:
        text = mmap.mmap(g.fileno(), 0, access=mmap.ACCESS_READ) if os.fstat(g.fileno()).st_size else None
        try:
            yield text if text is not None else b""
        finally:
            if text is not None:
                try:
                    text.close()
                except BufferError:                          # (an exception on its way up still holds views of the mapping)
                    pass


def _text_of(path_or_bytes):
    """context manager: a path -> _mapped(path); bytes / mmap / uint8 array -> the object itself, left as it is"""
    return _mapped(path_or_bytes) if isinstance(path_or_bytes, (str, os.PathLike)) else contextlib.nullcontext(path_or_bytes)


def line_cuts(text, n_parts, lo=0, hi=None):
    """n_parts + 1 offsets cutting text[lo:hi] into parts of whole lines of about equal bytes (lo and hi themselves must be line
    boundaries: 0, len(text) or an offset just behind a newline)."""
    hi = len(text) if hi is None else hi
    cuts = [lo]
    for k in range(1, n_parts):
        g = max(cuts[-1], lo + (hi - lo) * k // n_parts)
        nl = text.find(b"\n", g, hi)
        cuts.append(hi if nl < 0 else nl + 1)
    cuts.append(hi)
    return cuts


def ramp_cuts(text, lo, hi, chunk_bytes, first=None, growth=1.5):
    """offsets cutting text[lo:hi] into chunks of whole lines whose sizes grow from `first` bytes (default chunk_bytes / 4, at least 1 MB) by
    `growth` per chunk up to chunk_bytes: the pipeline's fill - nothing computes before the first chunk has been staged, copied, tokenised
    and encoded, and the forward of chunk 0 is issued behind the tokeniser of chunk 2 - shrinks with the first chunks (with equal 64 MB
    chunks the first forward of a 6 M-column contig started 4.0 ms into an 18.4 ms pass); growth 1.5 keeps the copy of the next, larger
    chunk shorter than the compute of the current one (H2D 0.018 ms / MB against 0.029 ms / MB of device work).  Where to start is a
    trade against the per-chunk issue cost (~0.3 ms of host time, ~30 launches): measured per contig of a run of contigs (the previous
    contig's last forwards cover most of the fill there) 18.9 / 17.6 / 17.3 / 17.6 / 18.0 ms starting at 4 / 8 / 16 / 32 / 64 MB."""
    chunk_bytes = max(1, int(chunk_bytes))
    if not first and os.environ.get("NSNP_RAMP_FIRST_MB"):           # (A/B measurements)
        first = int(float(os.environ["NSNP_RAMP_FIRST_MB"]) * (1 << 20))
    first = int(first) if first else max(min(chunk_bytes, 1 << 20), chunk_bytes // 4)
    cuts, size, target = [lo], float(min(first, chunk_bytes)), float(lo)
    while cuts[-1] < hi:
        target += size                               # (targets accumulate: the chunks average `size` bytes however long the lines are)
        g = max(int(target), cuts[-1] + 1)
        if g >= hi or hi - g < size / 2:             # (what is left is smaller than half a chunk: it joins this one)
            cuts.append(hi)
            break
        nl = text.find(b"\n", g - 1, hi)
        cuts.append(hi if nl < 0 else nl + 1)
        size = min(size * growth, float(chunk_bytes))
    return cuts


def halo_range(text, lo, hi, halo=16):
    """[lo, hi) grown by up to `halo` whole lines on either side -> (lo_ext, hi_ext, lines added in front, lines added behind)"""
    n_txt = len(text)
    a, n_lo = lo, 0
    while n_lo < halo and a > 0:
        nl = text.rfind(b"\n", 0, a - 1)
        a = nl + 1                                   # (-1 + 1 = 0 when the first line is reached)
        n_lo += 1
    b, n_hi = hi, 0
    while n_hi < halo and b < n_txt:
        nl = text.find(b"\n", b, n_txt)
        b = n_txt if nl < 0 else nl + 1
        n_hi += 1
    return a, b, n_lo, n_hi


def _cols_for(cap_bytes):
    """columns budgeted for a chunk of cap_bytes of text: one per 24 bytes (a samtools line at 30x is ~90 bytes; a valid line cannot
    be shorter than 10).  A chunk with more lines than that grows its buffer sets once, when the parser reports it (NSNP_HOST_ERANGE)."""
    return cap_bytes // 24 + 1024


class _HostSet:
    """pinned host buffers of one text chunk in flight (the parser writes straight into them, the copy engine reads them)"""
    def __init__(self, cap_bytes, cap_cols=None):
        import torch
        cap_cols = int(cap_cols or _cols_for(cap_bytes))
        self.pos = torch.empty(cap_cols, dtype=torch.int64, pin_memory=True)
        self.off = torch.empty(cap_cols + 1, dtype=torch.int64, pin_memory=True)
        self.bases = torch.empty(cap_bytes, dtype=torch.uint8, pin_memory=True)
        self.np = (self.pos.numpy(), self.off.numpy(), self.bases.numpy())
        self.h2d_done = None


class _DevSet:
    """device buffers of one text chunk in flight (filled by the copy stream, read by the chunk's encode / select / call rows)"""
    def __init__(self, cap_bytes, dev, cap_cols=None):
        import torch
        cap_cols = int(cap_cols or _cols_for(cap_bytes))
        self.pos = torch.empty(cap_cols, dtype=torch.int64, device=dev)
        self.off = torch.empty(cap_cols + 1, dtype=torch.int64, device=dev)
        self.bases = torch.empty(cap_bytes, dtype=torch.uint8, device=dev)
        self.free = None                               # event on the compute stream: the last kernels reading this set are done


def tokenise_mode(tokenise=None):
    """where the mpileup text is cut into columns: "device" (default: the raw text crosses PCIe and nsnp_mpileup_tokenise cuts it in HBM; the
    host only copies the text into pinned memory) or "host" (nsnp_mpileup_parse_into on the host cores; NSNP_TOKENISE=host)"""
    t = tokenise or os.environ.get("NSNP_TOKENISE", "device")
    if t not in ("device", "host"):
        raise ValueError(f"tokenise: 'device' or 'host', not {t!r}")
    return t


def stream_contig(model, text, contig, chr_seq, lo=0, hi=None, chunk_bytes=64 << 20, min_af=0.12, min_coverage=6, stats=None, on_rows=None,
                  tokenise=None, extended_bed=None, confident_bed=None, fai=None):
    beds = _contig_beds(extended_bed, confident_bed, contig, chr_seq, fai)
    with host.gc_paused():
        if tokenise_mode(tokenise) == "device":
            return _stream_contig_dev(model, text, contig, chr_seq, lo, hi, chunk_bytes, min_af, min_coverage, stats, on_rows, beds=beds)
        return _stream_contig(model, text, contig, chr_seq, lo, hi, chunk_bytes, min_af, min_coverage, stats, on_rows, beds=beds)


# ---- BED region filters (nanosnp_amd/bed.py; DNA_CreateCanSnpTensor -extended_confident_bed / -confident_bed) ---------------------------
def _contig_beds(extended_bed, confident_bed, contig, chr_seq, fai=None):
    """the two BED arguments of a pipeline call (None, a path, or {contig: intervals}) -> None without BEDs (the pipelines then issue
    exactly the launches they always issued), else (extended bitmap or None, confident bitmap or None) of this contig: host uint32 words"""
    if extended_bed is None and confident_bed is None:
        return None
    from . import bed
    n = int(chr_seq.size)
    mk = lambda b: None if b is None else bed.bed_bitmap(bed.contig_intervals(b, contig, n, fai), n)
    return mk(extended_bed), mk(confident_bed)


def _upload_pinned(model, attr, arrays, dtype, floor, dev, copy_stream, main):
    """What a contig brings along once - its reference sequence (attr "_seq_pin", uint8), its BED bitmaps ("_bed_pin", int32 words) - as
    device tensors.  arrays: numpy arrays of the type the torch `dtype` names, None where there is none; -> one tensor (or None) per array,
    each marked record_stream(main), for the compute stream is where it is read and given back.
    The values travel through a pinned buffer on the COPY stream: a copy from pageable memory on the compute stream would wait for
    everything queued there - the previous contig's last forward - and stall this thread for as long.  The compute stream waits for the copy.
    The pinned buffer is kept on the model as `attr`; one that is too small is replaced by one an eighth larger than needed, at least
    `floor` elements."""
    import torch
    total = sum(a.size for a in arrays if a is not None)
    pin, free = getattr(model, attr, None), getattr(model, attr + "_free", None)
    if pin is None or pin.numel() < total:
        pin, free = torch.empty(max(total + total // 8, floor), dtype=dtype, pin_memory=True), None
        setattr(model, attr, pin)
    if free is not None:
        free.synchronize()                             # (the previous contig's values have left the pinned buffer)
    out, o = [], 0
    with torch.cuda.stream(copy_stream):               # (allocated as the copy stream's memory: a block the compute stream has just freed may
        for a in arrays:                               # still be read by work queued there)
            if a is None:
                out.append(None)
                continue
            pin.numpy()[o:o + a.size] = a
            d = torch.empty(max(a.size, 1), dtype=dtype, device=dev)[:a.size]
            d.copy_(pin[o:o + a.size], non_blocking=True)
            d.record_stream(main)
            out.append(d)
            o += a.size
        free = torch.cuda.Event(); free.record(copy_stream)
    setattr(model, attr + "_free", free)
    main.wait_event(free)
    return out


def _upload_beds(model, beds, dev, copy_stream, main):
    """the contig's bitmaps -> device int32 tensors (None where there is none), once per contig, as the reference sequence travels"""
    import torch
    return _upload_pinned(model, "_bed_pin", [None if b is None else np.ascontiguousarray(b).view(np.int32) for b in beds], torch.int32, 1 << 16,
                          dev, copy_stream, main)


class _FilSet:
    """the columns of one chunk behind the extended-BED filter (nsnp_pileup_filter_columns): written and read on the compute stream alone.
    The bases lie behind a front pad (include/nanosnp.h: the encode of a chunk that keeps no byte reads the 16 bytes in front of them)."""
    def __init__(self, cap_cols, cap_bytes, dev):
        import torch
        from ._lib import Context
        self.pos = torch.empty(cap_cols, dtype=torch.int64, device=dev)
        self.off = torch.empty(cap_cols + 1, dtype=torch.int64, device=dev)
        self.ref = torch.empty(cap_cols, dtype=torch.uint8, device=dev)
        self.bases = torch.empty(Context.FILTER_FRONT_PAD + cap_bytes, dtype=torch.uint8, device=dev)[Context.FILTER_FRONT_PAD:]
        self.out = (self.pos, self.off, self.bases, self.ref)


class _FilKeySet(_FilSet):
    """_FilSet for the keyed columns of a whole-genome chunk (nsnp_pileup_filter_columns_keys: pos holds keys), plus the int32 per column that
    is compacted with them (the line_idx of the chunk's name table)"""
    def __init__(self, cap_cols, cap_bytes, dev):
        import torch
        super().__init__(cap_cols, cap_bytes, dev)
        self.aux = torch.empty(cap_cols, dtype=torch.int32, device=dev)
        self.out = self.out + (self.aux,)


class _TextSet:
    """one chunk of raw mpileup text in flight: pinned on the host (filled by the staging thread, read by the copy engine) or on the device
    (filled by the copy stream, read by the tokeniser)"""
    def __init__(self, cap_bytes, dev=None):
        import torch
        self.buf = torch.empty(cap_bytes, dtype=torch.uint8, **(dict(pin_memory=True) if dev is None else dict(device=dev)))
        self.np = self.buf.numpy() if dev is None else None
        self.h2d_done = None                           # host set: the copy engine has read it
        self.free = None                               # device set: the tokeniser has read it


class _ColSet:
    """the columns of one chunk on the device, as nsnp_mpileup_tokenise writes them and the encode reads them.  Sized for any text of
    cap_bytes (a line is at least 10 bytes, its column 5 shorter than the line): no growth path, nothing to re-run."""
    def __init__(self, cap_bytes, dev):
        import torch
        cc = cap_bytes // 10 + 2
        self.pos = torch.empty(cc, dtype=torch.int64, device=dev)
        self.off = torch.empty(cc + 1, dtype=torch.int64, device=dev)
        self.ref = torch.empty(cc, dtype=torch.uint8, device=dev)
        self.bases = torch.empty(cap_bytes, dtype=torch.uint8, device=dev)


_STREAM_STATS = ("parse_s", "h2d_s", "gpu_s", "tok_s", "text_bytes", "columns", "chunks", "setup_s", "wait_parse_s", "issue_s", "wait_counts_s", "drain_s")


def _stream_stats(stats):
    """the stats dict of a device-tokenised run, with every key the chunk loop adds to"""
    st = stats if stats is not None else {}
    for k in _STREAM_STATS:
        st.setdefault(k, 0.0)
    st["tokenise"] = "device"
    return st


def _count_slots(model, attr, n):
    """at least n pinned rows of four int64, kept on the model as `attr`: where the last launch of a chunk's stage leaves its counts"""
    import torch
    if len(getattr(model, attr, ())) < n:
        setattr(model, attr, torch.zeros((n, 4), dtype=torch.int64, pin_memory=True))
    return getattr(model, attr)


_ChunkSets = namedtuple("_ChunkSets", "ranges cap hsets tsets csets copy_stream main fresh")
# what the record kernels of a chunk read beside its counts and centres (device tensors; seq: the contig's sequence)
_ChunkColumns = namedtuple("_ChunkColumns", "bases off ref pos depth seq names")


class _NamesOverflow(Exception):
    """more lines of a chunk carry another token than the contig's name in column 0 than the name table holds (contig_to_bin runs again)"""
    def __init__(self, need):
        super().__init__(need)
        self.need = int(need)


def _text_chunk_sets(model, finder, lo, hi, chunk_bytes, dev):
    """The chunk plan of text[lo:hi] - ranges: (from, to, halo lines in front, halo lines behind) per chunk of whole lines; cap: the bytes a
    buffer must hold for the longest of them - and the buffer sets its chunks travel through, kept on the model (one call at a time per
    model) and built anew when a chunk no longer fits: pinned text sets, device text sets, column sets, and the copy stream, which has
    waited for the compute stream where it must.  -> _ChunkSets; fresh: the device sets are new."""
    import torch
    cuts = ramp_cuts(finder, lo, hi, int(chunk_bytes))
    ranges = [halo_range(finder, cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1) if cuts[k + 1] > cuts[k]]
    cap = max(b - a for a, b, _, _ in ranges) + 64
    # FOUR pinned text buffers (the staging thread works up to three chunks ahead of the tokeniser), THREE device text buffers (the copy of
    # chunk k + 1 is issued before the tokeniser of chunk k: the compute stream never waits for a copy that was only just issued - with
    # two buffers and the copy issued in the tokeniser's own iteration a 24 M-column contig ran at 65.7 ms against 48.7 ms of device time)
    hsets = getattr(model, "_text_host_sets", None)
    n_hsets, n_tsets, n_sets = min(4, len(ranges)), min(3, len(ranges)), min(3, len(ranges))
    if not hsets or min(s_.buf.numel() for s_ in hsets) < cap or len(hsets) < n_hsets:
        hsets = model._text_host_sets = [_TextSet(cap) for _ in range(n_hsets)]
        model._text_dev_sets = None
    # (model._text_dev_sets = None makes the next call build the device text AND column sets anew, as the host sets' growth above does;
    #  tests/test_gpu_predict.py uses that to make one model grow its sets again and again)
    tsets = getattr(model, "_text_dev_sets", None)
    fresh = not tsets or tsets[0].buf.device != dev or min(t_.buf.numel() for t_ in tsets) < cap or len(tsets) < n_tsets
    if fresh:
        tsets = model._text_dev_sets = [_TextSet(cap, dev) for _ in range(n_tsets)]
        model._col_dev_sets = [_ColSet(cap, dev) for _ in range(n_sets)]
        model._copy_stream = getattr(model, "_copy_stream", None) or host.copy_stream(dev)
    copy_stream = model._copy_stream
    main = torch.cuda.current_stream(dev)
    # (the sets keep their events from the previous call: a pinned buffer is rewritten only behind the copy that read it, a device text buffer
    # behind the tokeniser that read it - whichever call issued those; the column sets are written and read on the compute stream alone)
    if getattr(model, "_stream_main_id", None) != (main.device, main.stream_id):
        copy_stream.wait_stream(main)                  # (another compute stream than last time: its queued work may still read the device sets)
        model._stream_main_id = (main.device, main.stream_id)
    if fresh:
        # New device sets come out of the compute stream's pool: their blocks may be ones the previous contig's tensors gave back while its
        # last kernels (call_contigs defers them) are still queued there and still read them.  The compute stream's own later work is
        # ordered behind those kernels; the copy stream is not, and its first write into a new text buffer would be - so it waits once
        # for everything queued on the compute stream so far.  Nothing in the steady state: sets that are kept are not new.
        copy_stream.wait_stream(main)
    return _ChunkSets(ranges, cap, hsets, tsets, model._col_dev_sets, copy_stream, main, fresh)


def _run_text_chunks(sets, arr, st, tokenise, encode, calls):
    """The chunks of sets.ranges (_text_chunk_sets) of the text `arr` (numpy uint8), worked off four things at a time:

        worker thread   copies chunks k + 2 and k + 3 into two of four pinned text buffers (libnanosnp_host.so: nsnp_stage_values)
        copy stream     sends the text of chunk k + 1 (three device text buffers: a copy waits for the tokeniser three chunks back)
        compute stream  tokenise(k, text of chunk k on the device, column set)  the caller's tokeniser, its counts into the caller's pinned slot
                        encode(k, column set, n_lo, n_hi) of chunk k - 1: its line count came back through pinned memory while chunk k was being
                            issued; the caller reads it, refuses what it must, issues encode + select -> a job, or None without columns of its own
                        calls(k, job) of chunk k - 2, its site count likewise: forward + call rows; called for every chunk, in order

    so this thread never waits for work it has just issued, and the device never waits for this thread.  An exception - a caller's refusal
    of the text among them - leaves nothing queued behind it.  Returns, as soon as the last chunk is ISSUED, finalize(done): it waits for `done`
    (an event of the compute stream behind the last thing the caller issued) and the copy stream and adds the per-stage times to st; the
    buffer sets carry their events from call to call, so the next call may start before.  st["trace"], a list: gets (what, chunk, t0, t1)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    ranges, hsets, tsets, csets, copy_stream, main = sets.ranges, sets.hsets, sets.tsets, sets.csets, sets.copy_stream, sets.main
    trace = st.get("trace")
    t_enter = time.perf_counter()
    ev0 = torch.cuda.Event(enable_timing=True)
    if trace is not None:
        torch.cuda.synchronize(main.device); ev0.record(main); torch.cuda.synchronize(main.device)
    t_ev0 = time.perf_counter()
    st["setup_s"] += t_ev0 - t_enter                   # (the trace's two waits for the device belong to the setup, as they always did)
    tev = lambda: torch.cuda.Event(enable_timing=True)
    ev = [dict(h0=tev(), h1=tev(), t0=tev(), t1=tev(), a0=tev(), a1=tev(), b0=tev(), b1=tev()) for _ in ranges]

    def stage(k):
        t0 = time.perf_counter()
        a, b, _, _ = ranges[k]
        host.stage_values(hsets[k % len(hsets)].np, b - a, src=arr, src_off=a, src_dtype=np.uint8)
        t1 = time.perf_counter()
        if trace is not None:
            trace.append(("stage", k, t0, t1))
        return t1 - t0

    def wait_counts(event):
        t_w = time.perf_counter()
        event.synchronize()
        st["wait_counts_s"] += time.perf_counter() - t_w

    def second(k, cs, n_lo, n_hi, tok_done):
        """the second third of a chunk: its line count is on the host by now"""
        wait_counts(tok_done)
        ev[k]["a0"].record(main)
        job = encode(k, cs, n_lo, n_hi)
        ev[k]["a1"].record(main)
        sel_done = None
        if job is not None:
            sel_done = torch.cuda.Event(); sel_done.record(main)
        return k, job, sel_done

    def last(k, job, sel_done):
        """the last third of a chunk: its site count is on the host by now"""
        if sel_done is not None:
            wait_counts(sel_done)
        ev[k]["b0"].record(main)
        calls(k, job)
        ev[k]["b1"].record(main)

    pending, third = deque(), None
    with ThreadPoolExecutor(max_workers=1) as pool:
        futs = [pool.submit(stage, j) for j in range(min(3, len(ranges)))]

        def send(j):
            """the text of chunk j on its way: copy stream, behind the tokeniser of chunk j - 3 (the last reader of its device text buffer)"""
            t_w = time.perf_counter()
            t_stage = futs[j].result()
            t_s = time.perf_counter()
            st["wait_parse_s"] += t_s - t_w
            if trace is not None:
                trace.append(("main: wait stage", j, t_w, t_s))
            a_, b_, _, _ = ranges[j]
            n_ = b_ - a_
            hs, ts = hsets[j % len(hsets)], tsets[j % len(tsets)]
            st["parse_s"] += t_stage; st["text_bytes"] += n_; st["chunks"] += 1
            if ts.free is not None:
                copy_stream.wait_event(ts.free)
            with torch.cuda.stream(copy_stream):
                ev[j]["h0"].record(copy_stream)
                ts.buf[:n_].copy_(hs.buf[:n_], non_blocking=True)
                ev[j]["h1"].record(copy_stream)
            hs.h2d_done = ev[j]["h1"]
            if j + 3 < len(ranges):
                nxt = hsets[(j + 3) % len(hsets)]
                if nxt.h2d_done is not None:
                    nxt.h2d_done.synchronize()          # the copy engine is done with the buffer the staging thread is about to overwrite (chunk j - 1)
                futs.append(pool.submit(stage, j + 3))

        try:
            send(0)
            for k, (a, b, n_lo, n_hi) in enumerate(ranges):
                t_i = time.perf_counter()
                if k + 1 < len(ranges):
                    send(k + 1)                         # one chunk ahead of the tokeniser
                ts, cs = tsets[k % len(tsets)], csets[k % len(csets)]
                # ---- first third of chunk k on the compute stream: the tokeniser; lines / bytes / status land in pinned memory ----
                main.wait_event(ev[k]["h1"])
                ev[k]["t0"].record(main)
                tokenise(k, ts.buf[:b - a], cs)
                ev[k]["t1"].record(main)
                ts.free = ev[k]["t1"]
                tok_done = torch.cuda.Event(); tok_done.record(main)
                pending.append((k, cs, n_lo, n_hi, tok_done))
                # ---- second third of chunk k - 1, last third of chunk k - 2 ----
                nxt_third = second(*pending.popleft()) if len(pending) > 1 else None
                if third is not None:
                    last(*third)
                third = nxt_third
                st["issue_s"] += time.perf_counter() - t_i
                if trace is not None:
                    trace.append(("main: issue", k, t_i, time.perf_counter()))
            t_i = time.perf_counter()
            while pending or third is not None:
                nxt_third = second(*pending.popleft()) if pending else None
                if third is not None:
                    last(*third)
                third = nxt_third
            st["issue_s"] += time.perf_counter() - t_i
        except BaseException:
            # whatever ends the loop early, nothing queued may outlive the call: the pinned and device sets stay on the model for the next one
            t_d = time.perf_counter()
            for f_ in futs:
                f_.cancel()
            main.synchronize()
            copy_stream.synchronize()
            st["drain_s"] += time.perf_counter() - t_d
            raise

    def finalize(done):
        t_d = time.perf_counter()
        done.synchronize()
        copy_stream.synchronize()
        st["drain_s"] += time.perf_counter() - t_d
        if trace is not None:
            for k, e in enumerate(ev):
                for what, x0, x1 in (("h2d", "h0", "h1"), ("tokenise", "t0", "t1"), ("encode+select", "a0", "a1"), ("forward+rows", "b0", "b1")):
                    trace.append((what, k, t_ev0 + ev0.elapsed_time(e[x0]) * 1e-3, t_ev0 + ev0.elapsed_time(e[x1]) * 1e-3))
        for e in ev:
            st["h2d_s"] += e["h0"].elapsed_time(e["h1"]) * 1e-3
            tk = e["t0"].elapsed_time(e["t1"]) * 1e-3
            st["tok_s"] += tk; st["gpu_s"] += tk
            st["gpu_s"] += (e["a0"].elapsed_time(e["a1"]) + e["b0"].elapsed_time(e["b1"])) * 1e-3

    return finalize


def _stream_contig_dev(model, text, contig, chr_seq, lo, hi, chunk_bytes, min_af, min_coverage, stats, on_rows, defer=False, beds=None,
                       indel_min_af=None, records=None, name_cap=1024):
    """stream_contig with the text cut into columns ON THE DEVICE (nsnp_mpileup_tokenise).  The host touches every byte of the text once - a
    multi-threaded copy of the chunk (whole lines, 16 lines of halo either side, found by a few find / rfind calls) from the page cache
    into pinned memory - and the chunks are worked off four things at a time by _run_text_chunks, over the buffer sets of _text_chunk_sets;
    this function brings what belongs to ONE contig: its reference sequence and BED bitmaps on the device, the filter sets, the pinned
    count slots of its chunks and the three stage bodies.  Same rows as the host-parsed path (tests/test_gpu_predict.py); text the
    reference's reader aborts on is refused with the same errors.
    defer=True (call_contigs): returns (rows, done, finalize) as soon as the last chunk is ISSUED - `done` is an event behind the last kernel,
    finalize() waits for it and adds the per-stage times to stats - so that the next contig's text is staged, copied and tokenised while
    this one's last forward (1.4 ms of a 6 M-column contig's 15) still runs; the buffer sets carry their events from call to call.
    beds (_contig_beds; None: nothing below changes): with an extended bitmap every chunk's columns pass nsnp_pileup_filter_columns in front
    of the encode - the images of the chunk's own range stay on the device, the selection reads them there - and with a confident bitmap
    the encode is nsnp_pileup_encode_columns3.  The result does not depend on the cuts for texts with ASCENDING positions: 33 kept lines
    with consecutive positions are then 33 consecutive lines of the text, inside the 16-line halo; in a text whose positions repeat or step
    back they may lie further apart (the whole-array calls stay exact for any position sequence).
    records (contig_to_bin; None: nothing below changes): the third station issues no forward - records(chunk's arrays) is called for every
    chunk that owns sites and issues what it wants of them instead; no rows come back.  indel_min_af (None: min_af) goes to the encode."""
    import time
    import torch
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    finder, arr = _as_bytes_like(text)
    hi = arr.size if hi is None else hi
    st = _stream_stats(stats)
    t_enter = time.perf_counter()
    if hi <= lo:
        empty = torch.zeros((0, 13), dtype=torch.float64, device=dev)
        return (empty, None, lambda: None) if defer else empty
    sets = _text_chunk_sets(model, finder, lo, hi, chunk_bytes, dev)
    ranges, csets, copy_stream, main = sets.ranges, sets.csets, sets.copy_stream, sets.main
    meta_pin, tok_pin = _count_slots(model, "_meta_pin", len(ranges)), _count_slots(model, "_tok_meta_pin", len(ranges))
    n_seq = int(chr_seq.size)
    d_seq, = _upload_pinned(model, "_seq_pin", [chr_seq], torch.uint8, 1 << 20, dev, copy_stream, main)
    cov_idx = getattr(model, "_cov_idx", None)
    if cov_idx is None or cov_idx.device != dev:
        cov_idx = model._cov_idx = torch.tensor(list(COV_CHANNELS), dtype=torch.int64, device=dev)
    ext_bits = conf_bits = fsets = fmeta = None
    if beds is not None:
        ext_bits, conf_bits = _upload_beds(model, beds, dev, copy_stream, main)
        if ext_bits is not None:
            fsets = getattr(model, "_fil_dev_sets", None)
            if not fsets or fsets[0].pos.device != dev or fsets[0].pos.numel() < csets[0].pos.numel() or fsets[0].bases.numel() < csets[0].bases.numel():
                fsets = model._fil_dev_sets = [_FilSet(csets[0].pos.numel(), csets[0].bases.numel(), dev) for _ in range(3)]
                if not sets.fresh:
                    copy_stream.wait_stream(main)      # (new filter sets are new device sets: _text_chunk_sets says why the copy stream waits)
            fmeta = torch.zeros((len(ranges), 4), dtype=torch.int64, device=dev)
    rows_all = []

    # records: column 0 of every line against the contig's name, while the chunk's text is still on the device (the reference prints the
    # emitting line's token into the position string: nsnp_mpileup_line_names)
    names_pin = _count_slots(model, "_names_meta_pin", len(ranges)) if records is not None else None
    names_of = {}

    def tokenise(k, text_k, cs):
        ctx.mpileup_tokenise_into(text_k, d_seq, cs.pos, cs.off, cs.bases, cs.ref, tok_pin[k], stream=main)
        if records is not None:
            names_of[k] = ctx.mpileup_line_names(text_k, contig, int(text_k.numel()) // 10 + 2, name_cap, meta=names_pin[k], stream=main)[:2]

    def encode(k, cs, n_lo, n_hi):
        M, nb, status, _ = tok_pin[k].tolist()
        if status & ctx.TOK_EFORMAT:
            raise host.HostError(f"{contig}: malformed input (a line with fewer than five tab-separated fields)")
        if status & ctx.TOK_BLANK:
            raise host.HostError(f"{contig}: mpileup text holds empty line(s): malformed input (every line must be one pileup column)")
        if status & ctx.TOK_EPOS:
            raise ValueError(f"{contig}: position outside the reference sequence")
        if status:
            raise host.HostError(f"{contig}: tokeniser status {status}")
        own = M - n_lo - n_hi
        st["columns"] += own
        names = None
        if records is not None:
            names = names_of.pop(k)
            n_other, n_status, _, _ = names_pin[k].tolist()
            if n_status:
                raise _NamesOverflow(n_other)
            if n_other == 0:
                names = None                                 # (every line names the contig: the records carry the one name)
            elif ext_bits is not None:
                raise NotImplementedError(f"{contig}: lines with another name in column 0 under an extended BED (the filter does not carry them along)")
        if own <= 0:
            return None
        d_pos, d_off, d_bases, d_ref = cs.pos[:M], cs.off[:M + 1], cs.bases[:max(nb, 1)], cs.ref[:M]
        if ext_bits is not None:
            # the lines outside the extended BED leave the arrays; where the chunk's own range [n_lo, M - n_hi) lies among the kept
            # columns stays on the device (fmeta[k][2:])
            d_pos, d_off, d_bases, d_ref, _ = ctx.pileup_filter_columns(d_pos, d_off, d_bases, d_ref, ext_bits, n_seq, n_lo, M - n_hi,
                                                                        meta=fmeta[k], out=fsets[k % len(fsets)].out, stream=main)
        if conf_bits is not None:
            counts, depth, flags, _ = ctx.pileup_encode_columns3(d_bases, d_off, d_ref, d_pos, conf_bits, n_seq, min_af, min_coverage,
                                                                 want_max_del=False, indel_min_af=indel_min_af)
        else:
            counts, depth, flags = ctx.pileup_encode_columns(d_bases, d_off, d_ref, min_af, min_coverage, indel_min_af=indel_min_af)
        # selection + the run of the chunk's own sites in the list, written into pinned memory by the last of its four launches
        if ext_bits is not None:
            center = ctx.pileup_select_sites_range_dev(d_pos, flags, fmeta[k][2:], meta_pin[k], stream=main)
        else:
            center = ctx.pileup_select_sites_range(d_pos, flags, n_lo, M - n_hi, meta_pin[k], stream=main)
        if records is not None:
            return d_pos, counts, center, _ChunkColumns(d_bases, d_off, d_ref, d_pos, depth, d_seq, names)
        return d_pos, counts, center

    def calls(k, job):
        if job is None:
            return
        if records is not None:
            _, c_lo, c_hi, _ = meta_pin[k].tolist()
            if c_hi > c_lo:
                records(k, job[1], job[2][c_lo:c_hi], job[3], main)
            return
        d_pos, counts, center = job
        _, c_lo, c_hi, _ = meta_pin[k].tolist()
        if c_hi > c_lo:
            centers = center[c_lo:c_hi]
            gt, zy, ga, za, gm, zm = ctx.pileup_forward_windows_calls(counts, centers)
            rows_k = ctx.pileup_call_rows(counts, centers, d_pos, ga, za, gm, zm)                  # predict.py:52-65, one launch
            if on_rows is not None:
                on_rows(rows_k)
            else:
                rows_all.append(rows_k)

    st["setup_s"] += time.perf_counter() - t_enter
    finalize = _run_text_chunks(sets, arr, st, tokenise, encode, calls)
    rows = None if on_rows is not None else (torch.cat(rows_all) if rows_all else torch.zeros((0, 13), dtype=torch.float64, device=dev))
    done = torch.cuda.Event(); done.record(main)
    if defer:
        return rows, done, lambda: finalize(done)
    finalize(done)
    return rows


def _stream_contig(model, text, contig, chr_seq, lo, hi, chunk_bytes, min_af, min_coverage, stats, on_rows, beds=None):
    """The device part of stages s1 + s2 over the lines of text[lo:hi], chunk by chunk, three things at a time:

        worker thread   parses chunks k + 1 and k + 2 (libnanosnp_host.so, OpenMP, straight into one of three pinned buffer sets)
        copy stream     sends chunk k to the device (three device buffer sets: chunk k + 3 waits for the last readers of chunk k)
        compute stream  column encode -> site selection of chunk k, then PileupModel forward + argmax / max of chunk k - 1

    The number of selected sites is data: it comes back through a pinned buffer and is read ONE CHUNK LATER (the forward of chunk
    k - 1 is issued behind the encode of chunk k), so this thread never waits for work it has just issued and the device never
    waits for this thread.  Every chunk is parsed with 16 lines of halo on either side (re-parsed, not exchanged) and calls the
    sites centred in its own lines, so the result does not depend on where the cuts fall.
    Returns the call rows [n, 13] float64 (position, argmax / max of both heads, the eight coverage channels: all exact in float64)
    as a device tensor in position order - or, with on_rows, hands every chunk's rows to that callback as soon as they are issued
    and returns None.  stats (a dict) receives per-stage busy times (and, with a list under stats["trace"], the spans of every chunk's
    parse / copy / encode / forward on one clock: tools/probes/e2e_timeline.py).  The pinned and device buffer sets live on `model` between
    calls: one call at a time per model (use one model per thread)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    finder, arr = _as_bytes_like(text)
    hi = arr.size if hi is None else hi
    st = stats if stats is not None else {}
    for k in ("parse_s", "h2d_s", "gpu_s", "text_bytes", "columns", "chunks", "setup_s", "wait_parse_s", "issue_s", "wait_counts_s", "drain_s"):
        st.setdefault(k, 0.0)
    t_enter = time.perf_counter()
    if hi <= lo:
        return torch.zeros((0, 13), dtype=torch.float64, device=dev)
    n_chunks = max(1, -(-(hi - lo) // int(chunk_bytes)))
    cuts = line_cuts(finder, n_chunks, lo, hi)
    if n_chunks >= 3:
        # the pipeline's fill: nothing computes while the first chunk is parsed and copied - it is half a chunk (the other half goes
        # to a chunk of its own behind it)
        half = finder.find(b"\n", lo + (cuts[1] - lo) // 2, cuts[1])
        if half >= 0 and lo < half + 1 < cuts[1]:
            cuts = [lo, half + 1] + cuts[1:]
    ranges = [halo_range(finder, cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1) if cuts[k + 1] > cuts[k]]
    cap = max(b - a for a, b, _, _ in ranges) + 64
    # pinned buffers are expensive to create (page-locking): kept on the model between calls, with their device twins
    sets = getattr(model, "_host_sets", None)
    # THREE host sets: the parser works two chunks ahead of the copy engine (it never waits for this thread between two chunks)
    n_sets = min(3, len(ranges))
    if not sets or min(s_.bases.numel() for s_ in sets) < cap or len(sets) < n_sets:
        sets = [_HostSet(cap) for _ in range(n_sets)]
        model._host_sets = sets
        model._dev_sets = None
    dsets = getattr(model, "_dev_sets", None)
    # THREE device sets as well: with two, the copy of chunk k + 2 waits for the forward of chunk k (the last reader of its set) and the
    # encode of chunk k + 2 - in front of the forward of chunk k + 1 in stream order - waits for that copy: copies and forwards
    # alternated (tools/probes/e2e_timeline.py: 2.4 ms per chunk = copy 0.8 + encode 0.15 + forward 1.45); with three the copy runs beside
    # the forward of chunk k + 1
    if not dsets or len(dsets) < min(3, len(ranges)) or dsets[0].bases.device != dev or min(d_.bases.numel() for d_ in dsets) < cap:
        dsets = [_DevSet(cap, dev) for _ in range(min(3, len(ranges)))]
        model._dev_sets = dsets
        model._copy_stream = host.copy_stream(dev)
    if len(getattr(model, "_meta_pin", ())) < len(ranges):
        model._meta_pin = torch.zeros((len(ranges), 4), dtype=torch.int64, pin_memory=True)
    meta_pin = model._meta_pin
    copy_stream = model._copy_stream
    main = torch.cuda.current_stream(dev)
    for hs_ in sets:
        hs_.h2d_done = None
    for ds_ in dsets:
        ds_.free = None
    d_seq = torch.from_numpy(np.ascontiguousarray(chr_seq)).to(dev)
    seq_len = int(chr_seq.size)
    cov_idx = torch.tensor(list(COV_CHANNELS), dtype=torch.int64, device=dev)
    copy_stream.wait_stream(main)                      # (whatever the caller queued before us may still read the device sets)
    # BED bitmaps (_contig_beds; None: nothing below changes): the filter and the confident test run on the device in this mode too
    ext_bits, conf_bits = _upload_beds(model, beds, dev, copy_stream, main) if beds is not None else (None, None)
    fmeta = torch.zeros((len(ranges), 4), dtype=torch.int64, device=dev) if ext_bits is not None else None

    def parse(k):
        t0 = time.perf_counter()
        a, b, _, _ = ranges[k]
        try:
            out = host.mpileup_parse_range(arr, a, b, out=sets[k % len(sets)].np, strict_lines=True)
        except host.HostRangeError as e:
            # more (shorter) lines than budgeted: this set grows - the parser owns it right now (the copy engine was waited for before
            # this parse was submitted) - and the chunk is parsed again; the device twin grows on the main thread before the copy
            sets[k % len(sets)] = _HostSet(max(cap, e.n_bytes), e.n_cols + e.n_cols // 4 + 1024)
            out = host.mpileup_parse_range(arr, a, b, out=sets[k % len(sets)].np, strict_lines=True)
        pos = out[0]
        bad = bool(pos.size) and (int(pos.max()) > seq_len or int(pos.min()) < 1)
        t1 = time.perf_counter()
        if trace is not None:
            trace.append(("parse", k, t0, t1))
        return out, bad, t1 - t0

    rows_all = []
    trace = st.get("trace")                            # a list: receives (what, chunk, start, end) in host seconds; device spans are mapped onto the host clock
    ev0 = torch.cuda.Event(enable_timing=True)
    if trace is not None:
        torch.cuda.synchronize(dev); ev0.record(main); torch.cuda.synchronize(dev)
    t_ev0 = time.perf_counter()
    st["setup_s"] += time.perf_counter() - t_enter
    tev = lambda: torch.cuda.Event(enable_timing=True)
    ev = [dict(h0=tev(), h1=tev(), a0=tev(), a1=tev(), b0=tev(), b1=tev()) for _ in ranges]

    def calls_of(job):
        """the second half of a chunk: its site count is on the host by now"""
        k, M, n_lo, n_hi, ds, counts, center, sel_done, pos_k = job
        t_w = time.perf_counter()
        sel_done.synchronize()
        st["wait_counts_s"] += time.perf_counter() - t_w
        _, c_lo, c_hi, _ = meta_pin[k].tolist()
        ev[k]["b0"].record(main)
        if c_hi > c_lo:
            centers = center[c_lo:c_hi]                                                   # ascending: the chunk's own sites are one run
            gt, zy, ga, za, gm, zm = ctx.pileup_forward_windows_calls(counts, centers)
            # (index tensors made once, on the device: indexing with a Python list copies it from pageable memory every time, and
            # that copy waits for everything queued on the device - the forward just issued included)
            cov = counts.index_select(0, centers).index_select(1, cov_idx).to(torch.float64)      # predict.py:63
            f64 = lambda t: t.to(torch.float64)[:, None]
            rows_k = torch.cat([f64(pos_k.index_select(0, centers)), f64(ga), f64(za), f64(gm), f64(zm), cov], dim=1)
            if on_rows is not None:
                on_rows(rows_k)
            else:
                rows_all.append(rows_k)
        ev[k]["b1"].record(main)
        ds.free = torch.cuda.Event(); ds.free.record(main)

    job = None
    with ThreadPoolExecutor(max_workers=1) as pool:
        futs = [pool.submit(parse, j) for j in range(min(2, len(ranges)))]       # (one worker: the parses run one after the other)
        for k, (a, b, n_lo, n_hi) in enumerate(ranges):
            if job is not None and not futs[k].done() and os.environ.get("NSNP_PIPE_NO_EARLY_CALLS") != "1":      # (the variable: A/B measurements)
                # the parser is still busy with chunk k: the calls of chunk k - 1 go out now instead of behind the encode of chunk k
                # (at the front of the text this starts the first forward a parse earlier)
                t_i0 = time.perf_counter()
                calls_of(job); job = None
                st["issue_s"] += time.perf_counter() - t_i0
            t_w = time.perf_counter()
            (pos, col_off, bases), bad, t_parse = futs[k].result()
            t_i = time.perf_counter()
            st["wait_parse_s"] += t_i - t_w
            if trace is not None:
                trace.append(("main: wait parse", k, t_w, t_i))
            if bad:
                raise ValueError(f"{contig}: position outside the reference sequence")
            hs, ds = sets[k % len(sets)], dsets[k % len(dsets)]
            st["parse_s"] += t_parse; st["text_bytes"] += b - a; st["chunks"] += 1
            M, nb = int(pos.size), int(bases.size)
            if M + 1 > ds.off.numel() or nb > ds.bases.numel():
                torch.cuda.synchronize(dev)                       # (rare: every reader of the old set is done before it is dropped)
                ds = dsets[k % len(dsets)] = _DevSet(max(nb, ds.bases.numel()), dev, max(M + M // 4 + 1024, ds.pos.numel()))
            # ---- H2D on the copy stream, behind the last readers of this device set (chunk k - 2) ----
            if ds.free is not None:
                copy_stream.wait_event(ds.free)
            with torch.cuda.stream(copy_stream):
                ev[k]["h0"].record(copy_stream)
                ds.pos[:M].copy_(hs.pos[:M], non_blocking=True)
                ds.off[:M + 1].copy_(hs.off[:M + 1], non_blocking=True)
                ds.bases[:max(nb, 1)].copy_(hs.bases[:max(nb, 1)], non_blocking=True)
                ev[k]["h1"].record(copy_stream)
            hs.h2d_done = ev[k]["h1"]
            if k + 2 < len(ranges):
                nxt = sets[(k + 2) % len(sets)]
                if nxt.h2d_done is not None:
                    nxt.h2d_done.synchronize()          # the copy engine is done with the set the parser is about to overwrite (chunk k - 1)
                futs.append(pool.submit(parse, k + 2))
            # ---- first half of chunk k on the compute stream: encode + select, the counts on their way to the host ----
            main.wait_event(ev[k]["h1"])
            ev[k]["a0"].record(main)
            own = M - n_lo - n_hi
            st["columns"] += own
            nxt_job = None
            if own > 0:
                d_pos = ds.pos[:M]
                d_ref = d_seq[d_pos - 1]
                d_off, d_bases = ds.off[:M + 1], ds.bases[:max(nb, 1)]
                if ext_bits is not None:
                    d_pos, d_off, d_bases, d_ref, _ = ctx.pileup_filter_columns(d_pos, d_off, d_bases, d_ref, ext_bits, seq_len, n_lo, M - n_hi,
                                                                                meta=fmeta[k], stream=main)
                if conf_bits is not None:
                    counts, depth, flags, _ = ctx.pileup_encode_columns3(d_bases, d_off, d_ref, d_pos, conf_bits, seq_len, min_af, min_coverage,
                                                                         want_max_del=False)
                else:
                    counts, depth, flags = ctx.pileup_encode_columns(d_bases, d_off, d_ref, min_af, min_coverage)
                if ext_bits is not None:
                    center = ctx.pileup_select_sites_range_dev(d_pos, flags, fmeta[k][2:], meta_pin[k], stream=main)
                else:
                    center, n_sel = ctx.pileup_select_sites_async(d_pos, flags)
                    # halo columns belong to the neighbours: the chunk's own centres are [c_lo, c_hi) of the ascending list
                    meta = torch.stack([n_sel[0], (center < n_lo).sum(), (center < M - n_hi).sum(), n_sel[0]])
                    meta_pin[k].copy_(meta, non_blocking=True)
                sel_done = torch.cuda.Event(); sel_done.record(main)
                nxt_job = (k, M, n_lo, n_hi, ds, counts, center, sel_done, d_pos)
            else:
                ds.free = torch.cuda.Event(); ds.free.record(main)
            ev[k]["a1"].record(main)
            # ---- second half of chunk k - 1 ----
            if job is not None:
                calls_of(job)
            job = nxt_job
            st["issue_s"] += time.perf_counter() - t_i
            if trace is not None:
                trace.append(("main: issue", k, t_i, time.perf_counter()))
        if job is not None:
            t_i = time.perf_counter()
            calls_of(job)
            st["issue_s"] += time.perf_counter() - t_i
    t_d = time.perf_counter()
    torch.cuda.synchronize(dev)
    st["drain_s"] += time.perf_counter() - t_d
    if trace is not None:
        for k, e in enumerate(ev):
            for what, x0, x1 in (("h2d", "h0", "h1"), ("encode+select", "a0", "a1"), ("forward+rows", "b0", "b1")):
                try:
                    trace.append((what, k, t_ev0 + ev0.elapsed_time(e[x0]) * 1e-3, t_ev0 + ev0.elapsed_time(e[x1]) * 1e-3))
                except RuntimeError:
                    pass
    for e in ev:
        st["h2d_s"] += e["h0"].elapsed_time(e["h1"]) * 1e-3
        st["gpu_s"] += e["a0"].elapsed_time(e["a1"]) * 1e-3
        if e["b0"].query() and e["b1"].query():
            try:
                st["gpu_s"] += e["b0"].elapsed_time(e["b1"]) * 1e-3
            except RuntimeError:
                pass                                   # (a chunk without columns of its own never recorded its second half)
    if on_rows is not None:
        return None
    return torch.cat(rows_all) if rows_all else torch.zeros((0, 13), dtype=torch.float64, device=dev)


stream_contig.__doc__ = _stream_contig.__doc__


def _format_rows(r, contig, chr_seq, batch_size, score_mode, as_view=False, shard_dev=None, nthreads=None, ctx=None):
    """call rows [n, 13] float64 (a device tensor, a host tensor or a numpy array) -> (VCF text, rows written) of the reference's
    predict loop over consecutive batches.  shard_dev (the device the process group's collectives take their tensors on): the rows are
    one rank's share of the contig -> (this rank's text, its rows, sites of all ranks); every rank must call.  Device rows are cut into their typed columns ON the device (six small kernels, 41 B per
    site over the bus instead of 104 B and nine numpy passes)."""
    import torch
    if isinstance(r, torch.Tensor) and r.is_cuda and ctx is not None:
        # one kernel cuts the rows into their typed columns and writes them (41 B per site) straight into pinned host memory: no
        # device-to-host copy, so a text run keeps the copy engines to the text's way in (a D2H copy beside the H2D stream makes the HIP
        # runtime open further SDMA engines - 6-8 ms each - and was seen to leave later H2D traffic of the process on a slower one)
        n = int(r.shape[0])
        hb = getattr(ctx, "_rows_host", None)
        if hb is None or hb[0].numel() < n:
            cap = max(n + n // 4, 65536)
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
            hb = ctx._rows_host = (mk(cap, torch.int64), mk(cap, torch.uint8), mk(cap, torch.uint8), mk(cap, torch.float32), mk(cap, torch.float32),
                                   mk((cap, 8), torch.float32))
        s_ = torch.cuda.current_stream(r.device)
        ctx.pileup_rows_unpack(r.contiguous(), hb, stream=s_)
        s_.synchronize()
        site_pos, ga, za, gm, zm = (t[:n].numpy() for t in hb[:5])
        cov = hb[5][:n].numpy()
    elif isinstance(r, torch.Tensor):
        site_pos = r[:, 0].to(torch.int64).cpu().numpy()
        ga, za = r[:, 1].to(torch.uint8).cpu().numpy(), r[:, 2].to(torch.uint8).cpu().numpy()
        gm, zm = r[:, 3].to(torch.float32).cpu().numpy(), r[:, 4].to(torch.float32).cpu().numpy()
        cov = r[:, 5:13].to(torch.float32).contiguous().cpu().numpy()
    else:
        site_pos = r[:, 0].astype(np.int64)
        ga, za, gm, zm = r[:, 1].astype(np.uint8), r[:, 2].astype(np.uint8), r[:, 3].astype(np.float32), r[:, 4].astype(np.float32)
        cov = r[:, 5:13].astype(np.float32)
    n = site_pos.shape[0]
    site_ref = chr_seq[site_pos - 1] & 0xDF                                  # make_predict_data/main.cpp:91 upper-cases
    first, n_total, heads = 0, n, None
    if shard_dev is not None:
        # one rank's rows of a sharded contig: the batches run over the site list of ALL ranks - where this rank's rows start in it
        # and the ten argmax values its rows may read from a batch that starts on another rank (two small collectives)
        from .dist import batch_heads, site_offsets
        first, n_total = site_offsets(n, shard_dev)
        heads = batch_heads(ga, first, n_total, batch_size, shard_dev)
    # the VCF rows depend on the batch boundary: one native call formats every batch (OpenMP over the batches)
    text, n_rows = host.vcf_format_batches(host.ContigTable([contig]), np.zeros(n, np.int32), site_pos, site_ref, ga, za, gm, zm, cov,
                                           batch_size=batch_size, score_mode=score_mode, as_view=as_view, first=first, n_total=n_total, heads=heads,
                                           nthreads=nthreads)
    return (text, n_rows) if shard_dev is None else (text, n_rows, n_total)


def _call_contig_rows_beside(model, mpileup_text, contig, chr_seq, min_af, min_coverage, batch_size, score_mode, chunk_bytes, stats, tokenise=None,
                             **bed_kw):
    """call_contig for one process with the rows of finished chunks formatted on a writer thread while later chunks compute: every
    chunk's call rows travel to a pinned buffer of their own behind the chunk's forward; the writer formats the COMPLETE batches of
    `batch_size` sites that have arrived (the reference's rows depend on the batch a site falls into: predict.py:102-125) with a
    quarter of the host threads and carries the rest over; what is left when the last chunk is back is formatted on all threads.
    Byte-identical to formatting all rows at the end (tests/test_gpu_predict.py)."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    pins = getattr(model, "_rows_pins", None)
    if pins is None:
        pins = model._rows_pins = []
    events, sizes, pieces = [], [], []
    state = dict(carry=np.empty((0, 13), np.float64), rows=0, busy=0.0)
    few = max(1, host.lib().nsnp_host_threads() // 4)

    def fmt(r, nthreads):
        t0 = time.perf_counter()
        site_pos = r[:, 0].astype(np.int64)
        text, n_rows = host.vcf_format_batches(host.ContigTable([contig]), np.zeros(len(r), np.int32), site_pos, chr_seq[site_pos - 1] & 0xDF,
                                               r[:, 1].astype(np.uint8), r[:, 2].astype(np.uint8), r[:, 3].astype(np.float32), r[:, 4].astype(np.float32),
                                               r[:, 5:13].astype(np.float32), batch_size=batch_size, score_mode=score_mode, nthreads=nthreads)
        pieces.append(text); state["rows"] += n_rows; state["busy"] += time.perf_counter() - t0

    def work(k):
        events[k].synchronize()
        got = pins[k][:sizes[k]].numpy()
        c = np.concatenate([state["carry"], got]) if len(state["carry"]) else got
        full = len(c) // batch_size * batch_size
        if full:
            fmt(c[:full], few)
        state["carry"] = c[full:].copy()

    with ThreadPoolExecutor(max_workers=1) as writer:
        futs = []

        def on_rows(rows_k):
            k, n = len(events), int(rows_k.shape[0])
            if k >= len(pins):
                pins.append(torch.empty((max(n + n // 4, 4096), 13), dtype=torch.float64, pin_memory=True))
            elif pins[k].shape[0] < n:
                pins[k] = torch.empty((n + n // 4, 13), dtype=torch.float64, pin_memory=True)
            pins[k][:n].copy_(rows_k, non_blocking=True)
            ev = torch.cuda.Event(blocking=True); ev.record()
            events.append(ev); sizes.append(n)
            futs.append(writer.submit(work, k))

        stream_contig(model, mpileup_text, contig, chr_seq, 0, None, chunk_bytes, min_af, min_coverage, stats, on_rows=on_rows, tokenise=tokenise,
                      **bed_kw)
        t0 = time.perf_counter()
        for f in futs:
            f.result()
        if len(state["carry"]):
            fmt(state["carry"], 0)
        n_sites = int(sum(sizes))
        text = b"".join(pieces)
        if stats is not None:
            stats["vcf_s"] = stats.get("vcf_s", 0.0) + time.perf_counter() - t0          # what the caller still waits for behind the last chunk
            stats["vcf_beside_s"] = stats.get("vcf_beside_s", 0.0) + state["busy"]
            stats["sites"] = stats.get("sites", 0) + n_sites
            stats["vcf_rows"] = stats.get("vcf_rows", 0) + state["rows"]
    return text, n_sites, state["rows"]


def call_contig(model, mpileup_text, contig: str, chr_seq: np.ndarray, min_af=0.12, min_coverage=6,
                batch_size=1000, score_mode=host.SCORE_FLOAT64, chunk_bytes=64 << 20, stats=None, rows_beside=None, tokenise=None,
                extended_bed=None, confident_bed=None, fai=None):
    """One contig: returns (vcf_rows: bytes-like - a memoryview of the formatter's buffer, no copy; bytes(...) it to keep it -, n_sites, n_rows).  model: pileup_model.LSTMNetwork; mpileup_text: bytes, mmap or a
    numpy uint8 array holding the contig's samtools-mpileup text.  tokenise: "device" (default) / "host" (tokenise_mode).
    extended_bed / confident_bed: the reference's -extended_confident_bed / -confident_bed region filters (nanosnp_amd/bed.py), each None,
    the path of a BED file, or {contig: intervals [n, 2] of 0-based half-open (from, to)}; fai: the reference index (a {name: length} dict or
    .fai text) a BED path is checked against - without it only this contig's lines are read and checked.  Lines outside the extended BED
    are dropped on the device before the window rule sees them; a column is a candidate only when the confident BED holds a base of
    [pos - 1, pos + its longest deletion + 1).  With both None the call issues exactly the launches it issued without these arguments.

    The text is worked off in chunks of whole lines (stream_contig: parse of chunk k + 1 on the host beside the device work of
    chunk k).  Under an initialised torch.distributed process group (one process per GPU, torchrun) the TEXT is statically sharded:
    rank r parses and calls only the lines of its byte range (cut at line boundaries; 16 lines of halo re-parsed, not exchanged) and
    formats the rows of ITS sites exactly as a single process would format them (the reference's batches of `batch_size` sites run
    over the whole site list: dist.site_offsets + dist.batch_heads hand a rank the little it needs of the others); the text is
    gathered to rank 0 in rank = position order.  Ranks other than 0 return (b"", n_sites_total, 0)."""
    import time
    import torch
    import torch.distributed as tdist
    from .dist import gather_text
    ctx = model.ctx
    finder, arr = _as_bytes_like(mpileup_text)
    sharded = tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
    rank, world = (tdist.get_rank(), tdist.get_world_size()) if sharded else (0, 1)
    if rows_beside is None:
        rows_beside = os.environ.get("NSNP_ROWS_BESIDE", "0") == "1"
    if rows_beside and not sharded:
        return _call_contig_rows_beside(model, mpileup_text, contig, chr_seq, min_af, min_coverage, batch_size, score_mode, chunk_bytes, stats, tokenise,
                                        extended_bed=extended_bed, confident_bed=confident_bed, fai=fai)
    cuts = line_cuts(finder, world, 0, arr.size)
    rows = stream_contig(model, mpileup_text, contig, chr_seq, cuts[rank], cuts[rank + 1], chunk_bytes, min_af, min_coverage, stats, tokenise=tokenise,
                         extended_bed=extended_bed, confident_bed=confident_bed, fai=fai)
    if sharded:
        # every rank formats ITS rows (on its own host cores, exactly as the single process would format them: _format_rows), the text
        # - about 60 B per row, half of what the calls take - travels to rank 0 in one rooted gather
        backend_dev = torch.device("cuda", ctx.device) if tdist.get_backend() == "nccl" else "cpu"
        t0 = time.perf_counter()
        text, n_rows, n_sites = _format_rows(rows, contig, chr_seq, batch_size, score_mode, as_view=True, shard_dev=backend_dev, ctx=ctx)
        t1 = time.perf_counter()
        cnt = torch.tensor([n_rows], dtype=torch.int64, device=backend_dev)
        tdist.all_reduce(cnt)
        text = gather_text(text, backend_dev)
        if stats is not None:
            stats["vcf_s"] = stats.get("vcf_s", 0.0) + t1 - t0
            stats["gather_s"] = stats.get("gather_s", 0.0) + time.perf_counter() - t1
            stats["sites"] = stats.get("sites", 0) + int(rows.shape[0])
            stats["vcf_rows"] = stats.get("vcf_rows", 0) + n_rows
        return (text, n_sites, int(cnt.item())) if rank == 0 else (b"", n_sites, 0)
    # (formatting the rows of finished chunks on a worker thread while later chunks compute - rows_beside=True,
    # _call_contig_rows_beside - is built, byte-identical and SLOWER: round 3 with the 34 ms formatter 162 against 75 ms per 6 M-column
    # contig; round 5 with the 2.4 ms formatter on a quarter of the threads 27.6-28.4 against 22.5 ms (median of 30 steps, A/B/A/B on
    # one box): the per-chunk D2H copies and the writer's numpy passes cost the issuing thread 5 ms (GIL, copy-engine calls) to save
    # 2.4 ms behind the last chunk.  Off by default.)
    n_sites = int(rows.shape[0])
    if n_sites == 0:
        return b"", 0, 0
    t0 = time.perf_counter()
    text, n_rows = _format_rows(rows, contig, chr_seq, batch_size, score_mode, as_view=True, ctx=ctx)
    if stats is not None:
        stats["vcf_s"] = stats.get("vcf_s", 0.0) + time.perf_counter() - t0
        stats["sites"] = stats.get("sites", 0) + n_sites
        stats["vcf_rows"] = stats.get("vcf_rows", 0) + n_rows
    return text, n_sites, n_rows


def call_contigs(model, items, out, min_af=0.12, min_coverage=6, batch_size=1000, score_mode=host.SCORE_FLOAT64, chunk_bytes=64 << 20, stats=None,
                 extended_bed=None, confident_bed=None, fai=None):
    """A run over several contigs.  items: iterable of (name, mpileup text - bytes / mmap / uint8 array -, reference sequence uint8); out:
    a binary file object the rows are appended to (None on ranks other than 0).  Returns (sites, rows).
    One process: the rows of contig c are cut, brought to the host (on a stream of their own), formatted and written on a WRITER thread
    while contig c + 1 streams - formatting + writing is 4-5 ms behind every 6 M-column contig otherwise, a fifth of its time - on a
    quarter of the host threads (the parser keeps the rest busy; the last contig's rows get them all).  Under a process group the
    contigs run one after the other through call_contig (its collectives stay on the issuing thread).
    extended_bed / confident_bed / fai: as for call_contig (a BED path is read once for the run when fai is given); under a process group they
    pass straight through to every rank's call."""
    import time
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    import torch
    import torch.distributed as tdist
    sharded = tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
    st = stats if stats is not None else {}
    n_sites = n_rows = 0
    if fai is not None:                                     # (a BED path: parsed once, against the whole index)
        from . import bed as _bed
        extended_bed, confident_bed = (b if b is None or isinstance(b, dict) else _bed.load_bed(b, fai) for b in (extended_bed, confident_bed))
    if sharded:
        for name, text, seq in items:
            rows_text, ns, nr = call_contig(model, text, name, seq, min_af, min_coverage, batch_size, score_mode, chunk_bytes, stats,
                                            extended_bed=extended_bed, confident_bed=confident_bed, fai=fai)
            if out is not None:
                out.write(rows_text)
            n_sites += ns; n_rows += nr
        return n_sites, n_rows
    dev = torch.device("cuda", model.ctx.device)
    side = getattr(model, "_rows_stream", None)
    if side is None:
        from . import _lib
        side = model._rows_stream = torch.cuda.Stream(dev)
        model._rows_ctx = _lib.Context(model.ctx.device)     # the writer thread's OWN context (a context serves one host thread at a time)
    wctx = model._rows_ctx
    few = max(1, host.lib().nsnp_host_threads() // 4)

    def finish(rows, name, seq, last, done=None):
        if done is not None:
            done.synchronize()                              # (the contig's last kernels: its stream call returned when they were issued)
        t0 = time.perf_counter()
        with torch.cuda.stream(side):                       # (the rows are complete: behind `done`, or behind stream_contig's own synchronize)
            text, nr = _format_rows(rows, name, seq, batch_size, score_mode, as_view=True, nthreads=0 if last else few, ctx=wctx)
        t1 = time.perf_counter()
        if out is not None:
            out.write(text)
        st["vcf_s"] = st.get("vcf_s", 0.0) + t1 - t0
        st["write_s"] = st.get("write_s", 0.0) + time.perf_counter() - t1
        return nr

    it = iter(items)
    nxt = next(it, None)
    pending = deque()
    on_device = tokenise_mode() == "device"
    finals = []
    with host.gc_paused(), ThreadPoolExecutor(max_workers=1) as writer:
        try:
            while nxt is not None:
                name, text, seq = nxt
                done = None
                if on_device:
                    # returns when the contig's last chunk is issued: the next contig's text is on its way while this one's tail computes
                    rows, done, fin = _stream_contig_dev(model, text, name, seq, 0, None, chunk_bytes, min_af, min_coverage, stats, None, defer=True,
                                                         beds=_contig_beds(extended_bed, confident_bed, name, seq, fai))
                    finals.append(fin)
                else:
                    rows = stream_contig(model, text, name, seq, 0, None, chunk_bytes, min_af, min_coverage, stats,
                                         extended_bed=extended_bed, confident_bed=confident_bed, fai=fai)
                nxt = next(it, None)
                n_sites += int(rows.shape[0])
                st["sites"] = st.get("sites", 0) + int(rows.shape[0])
                if rows.shape[0]:
                    pending.append(writer.submit(finish, rows, name, seq, nxt is None, done))
                while len(pending) > 1 or (nxt is None and pending):          # at most one contig's rows behind the streaming one
                    t_w = time.perf_counter()
                    n_rows += pending.popleft().result()
                    st["wait_rows_s"] = st.get("wait_rows_s", 0.0) + time.perf_counter() - t_w
        finally:
            for fin in finals:                                                 # (per-stage times of the deferred contigs; waits for their last kernels)
                fin()
    st["vcf_rows"] = st.get("vcf_rows", 0) + n_rows
    return n_sites, n_rows


def call_variants(model, contigs, fasta_path, fai_text, output_file, **kw):
    """contigs: iterable of (name, path to <name>.mpileup).  Writes pileup.vcf (rank 0 only under torch.distributed: see
    call_contig); returns total rows.  The contigs are one run (call_contigs): the rows of one are written while the next streams.
    extended_bed= / confident_bed= (call_contig) are checked against fai_text."""
    import torch.distributed as tdist
    root = not (tdist.is_available() and tdist.is_initialized()) or tdist.get_rank() == 0
    maps = []

    def items():
        for name, path in contigs:
            seq = host.fasta_load_contig(fasta_path, name)
            g = open(path, "rb")
            size = os.fstat(g.fileno()).st_size
            text = mmap.mmap(g.fileno(), 0, access=mmap.ACCESS_READ) if size else b""       # parsed in place, never copied
            maps.append((g, text if size else None))
            yield name, text, seq

    f = open(output_file, "wb") if root else None
    try:
        if root:
            f.write(host.vcf_header(fai_text).encode())
        if kw.get("extended_bed") is not None or kw.get("confident_bed") is not None:
            kw.setdefault("fai", fai_text)
        return call_contigs(model, items(), f, **kw)[1]
    finally:
        if f:
            f.close()
        for g, text in maps:
            if text is not None:
                try:
                    text.close()
                except BufferError:                  # (an exception on its way up still holds views of the mapping)
                    pass
            g.close()


# ---- .pd.bin site files -> pileup.vcf, streamed (PileupModel/predict.py:37-195 over PredictDataset files) ------------------------------
class _SiteSet:
    """buffers of one pass of a site file in flight: the [P,33,18] window matrices (as bytes: int16 or int32 views per pass)"""
    def __init__(self, P, dev=None):
        import torch
        kw = dict(pin_memory=True) if dev is None else dict(device=dev)
        self.P = P
        self.x = torch.empty(P * 33 * 18 * 4, dtype=torch.uint8, **kw)
        self.h2d_done = None
        self.free = None


def predict_pileup_bins(model, testing_paths, fai_text, output_file, batch_size=1000, score_mode=host.SCORE_FLOAT64, pass_sites=65536,
                        narrow=True, stats=None, distributed=True):
    with host.gc_paused():                             # (a generation-2 pass of the interpreter's collector sat in the set-up of a run: 38 ms)
        return _predict_pileup_bins(model, testing_paths, fai_text, output_file, batch_size, score_mode, pass_sites, narrow, stats, distributed)


def _predict_pileup_bins(model, testing_paths, fai_text, output_file, batch_size, score_mode, pass_sites, narrow, stats, distributed):
    """The reference's ``predict(model, testing_paths, reference_index_file, batch_size, output_file, device)`` (PileupModel/predict.py:
    37-195) over this repository's ``.pd.bin`` site files (sitefile.write_pileup_bin / pd_to_bin: the arrays of make_bin_predict_data.py:
    90-100): every file's windows are STREAMED - a worker thread `pread`s passes of `pass_sites` windows from the page cache into one of
    three pinned sets on all host cores (int16 counts as they are; the int32 counts of a reference-layout file narrowed to int16 on the
    way when they fit - they do: half the bytes over PCIe - else int32) and parses the ``ctg:pos:ref33`` fields natively (dataset.py:127-132), a copy stream sends the pass, the compute stream
    runs the PileupModel forward whose heads kernel writes argmax / max (10 bytes per site) straight into pinned host memory (the coverage
    slice of predict.py:63 is taken from the staged pass on the host: the H2D copy of a pass is the only copy-engine work); the
    files are one pipeline, and the rows of a file are formatted (one native call over the reference's batches of `batch_size` sites,
    which restart with every file as its DataLoader does) and appended on a writer thread while the next file computes.
    testing_paths: a list of paths, or a directory (its ``*.bin`` files in os.listdir order: predict.py:215).  Returns rows written.
    Under torch.distributed (one process per GPU) every rank works on its shard_range of every file's windows, cut at multiples of
    batch_size: the reference's batches run over the whole file, so a rank owns whole batches and formats its rows beside its compute as
    the single process does; the TEXT travels to rank 0 in one rooted gather behind the last file and rank 0 writes it in file, rank
    order (the other ranks return 0).  distributed=False: this process alone does the whole job even inside a process group."""
    import threading
    import time
    from concurrent.futures import ThreadPoolExecutor
    import torch
    import torch.distributed as tdist
    from . import sitefile
    from .dist import gather_text, shard_range
    from .hap_pipeline import _LocalNames
    t_begin = time.perf_counter()
    sharded = bool(distributed) and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1
    rank, world = (tdist.get_rank(), tdist.get_world_size()) if sharded else (0, 1)
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    st = stats if stats is not None else {}
    for k in ("stage_s", "h2d_s", "gpu_s", "vcf_s", "bytes_h2d", "sites", "passes", "passes_int16", "wait_stage_s", "issue_s", "drain_s", "stage_values_s",
              "stage_coverage_s", "stage_fields_s", "gpu_idle_s", "setup_s", "account_s"):
        st.setdefault(k, 0.0)
    if isinstance(testing_paths, (str, os.PathLike)):
        d = str(testing_paths)
        paths = [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".bin")] if os.path.isdir(d) else [d]
    else:
        paths = [str(p) for p in testing_paths]
    files = []
    for p in paths:                                    # every header is checked before a descriptor is opened or a row is written
        idx = sitefile.array_index(p)
        if ("position_matrix" not in idx or "position" not in idx or idx["position_matrix"][0] not in (np.dtype(np.int32), np.dtype(np.int16))
                or idx["position_matrix"][1][1:] != (33, 18)):
            raise sitefile.SiteFileError(f"{p}: not a pileup site file (position_matrix int16 / int32 [N,33,18] + position)")
        n_file = int(idx["position_matrix"][1][0])
        # this rank's windows of the file: [lo, hi) (everything without a process group), cut at multiples of batch_size: the reference's batches
        # run over the whole file, so every rank owns WHOLE batches and formats its rows without a word from the others
        lo, hi = shard_range(n_file, rank, world, align=int(batch_size))
        files.append(dict(path=p, n_file=n_file, lo=lo, n=hi - lo, x_off=idx["position_matrix"][2], fd=-1,
                          elem=idx["position_matrix"][0].itemsize,
                          position=sitefile.read_arrays(p, mmap=True)["position"]))
    P = int(max(1, pass_sites))
    seg_off = np.concatenate([[0], np.cumsum([f["n"] for f in files])]).astype(np.int64)
    n_total = int(seg_off[-1])
    passes = []                                                # (file, first window, end - ABSOLUTE indices in the file -, offset among this rank's sites)
    for fi, f in enumerate(files):
        a = f["lo"]
        while a < f["lo"] + f["n"]:
            b = min(f["lo"] + f["n"], a + (max(1, P // 4) if not passes and f["n"] > P else P))   # the very first pass: a quarter (the pipeline's fill)
            passes.append((fi, a, b, int(seg_off[fi]) + a - f["lo"]))
            a = b
    last_pass_of = {fi: k for k, (fi, _, _, _) in enumerate(passes)}
    names = _LocalNames()
    total_rows = 0
    kept = {}                                                  # sharded: the rows (text) of every file stay on this rank until the gather
    out = open(output_file, "wb") if rank == 0 else None
    try:
        for f in files:
            f["fd"] = os.open(f["path"], os.O_RDONLY)
        if out:
            out.write(host.vcf_header(fai_text).encode())
        if passes:
            n_sets = min(3, len(passes))
            hsets = getattr(model, "_site_host_sets", None)
            if not hsets or len(hsets) < n_sets or hsets[0].P < P:
                hsets = [_SiteSet(P) for _ in range(n_sets)]
                model._site_host_sets = hsets
                model._site_dev_sets = [_SiteSet(P, dev) for _ in range(n_sets)]
                model._site_copy_stream = host.copy_stream(dev)
            dsets, copy_stream = model._site_dev_sets, model._site_copy_stream
            main = torch.cuda.current_stream(dev)
            for s_ in hsets:
                s_.h2d_done = None
            for s_ in dsets:
                s_.free = None
            copy_stream.wait_stream(main)
            # pinned result arrays: one slot per file in flight (computing / being written / next), not one per run - pinning memory costs
            # about 0.5 ms per MB and a run may hold hundreds of files
            max_n = max(f["n"] for f in files)
            n_slots = 3
            res = getattr(model, "_site_results", None)
            if res is None or res["ga"].numel() < n_slots * max_n:
                mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
                res = dict(ga=mk(n_slots * max_n, torch.uint8), za=mk(n_slots * max_n, torch.uint8), gm=mk(n_slots * max_n, torch.float32),
                           zm=mk(n_slots * max_n, torch.float32))
                model._site_results = res
            pos_all = np.empty(n_total, np.int64); ctg_all = np.empty(n_total, np.int32); refb_all = np.empty(n_total, np.uint8)
            cov_all = np.empty((n_total, len(COV_CHANNELS)), np.float32)
            centers = (torch.arange(P, dtype=torch.int64, device=dev) * 33 + 16).contiguous()
            # the rows of a file have a whole file's compute time to be written: a quarter of the host threads, the staging keeps the rest busy
            writer_threads = max(1, host.lib().nsnp_host_threads() // 4)
            elem = [2 if narrow else 4]                 # int16 until a pass does not fit (then int32 for the rest of the run)
            lock = threading.Lock()

            def stage(k):
                t0 = time.perf_counter()
                fi, a, b, o = passes[k]
                f, m = files[fi], b - a
                hs = hsets[k % n_sets]
                e = 2 if f["elem"] == 2 else elem[0]
                v = hs.x.numpy()[:m * 594 * e].view(np.int16 if e == 2 else np.int32)
                if f["elem"] == 2:                      # int16 on disk (sitefile.write_pileup_bin's default): straight into the pinned set
                    host.stage_values(v, m * 594, fd=f["fd"], src_off=f["x_off"] + a * 594 * 2, src_dtype=np.int16)
                elif host.stage_values(v, m * 594, fd=f["fd"], src_off=f["x_off"] + a * 594 * 4):
                    with lock:
                        elem[0] = 4                     # a count beyond int16 (never at real coverage): this pass and the later ones go as int32
                    e = 4
                    v = hs.x.numpy()[:m * 594 * 4].view(np.int32)
                    host.stage_values(v, m * 594, fd=f["fd"], src_off=f["x_off"] + a * 594 * 4)
                t1 = time.perf_counter()
                host.window_channels(v, m, 16, COV_CHANNELS, out=cov_all[o:o + m])      # predict.py:63, from the staged pass: no D2H carries it
                t2 = time.perf_counter()
                fields = np.asarray(f["position"][a:b]).reshape(m, -1)
                p_, c_, r_ = host.parse_ctg_pos_ref(fields, names.table)
                while (c_ < 0).any():                   # a contig not seen before: one name per round (contigs are few, the parse is native)
                    names.add_names([bytes(fields[int(np.argmax(c_ < 0))]).rstrip(b"\0").strip().split(b":")[0].decode()])
                    p_, c_, r_ = host.parse_ctg_pos_ref(fields, names.table)
                pos_all[o:o + m] = p_; ctg_all[o:o + m] = c_; refb_all[o:o + m] = r_
                t3 = time.perf_counter()
                st["stage_values_s"] += t1 - t0; st["stage_coverage_s"] += t2 - t1; st["stage_fields_s"] += t3 - t2
                return e, t3 - t0

            def rows_of(fi, done):
                """writer thread: the VCF rows of file fi (the reference's batches restart with every file)"""
                nonlocal total_rows
                if done is not None:
                    done.synchronize()
                t0 = time.perf_counter()
                o0, o1 = int(seg_off[fi]), int(seg_off[fi + 1])
                r0 = (fi % n_slots) * max_n
                r1 = r0 + (o1 - o0)
                if o1 > o0:
                    text, rows = host.vcf_format_batches(names.table, ctg_all[o0:o1], pos_all[o0:o1], refb_all[o0:o1], res["ga"][r0:r1].numpy(),
                                                         res["za"][r0:r1].numpy(), res["gm"][r0:r1].numpy(), res["zm"][r0:r1].numpy(),
                                                         cov_all[o0:o1], batch_size=batch_size, score_mode=score_mode, as_view=True,
                                                         nthreads=writer_threads if fi + 1 < len(files) else 0,   # the last file: nothing else runs
                                                         first=files[fi]["lo"], n_total=files[fi]["n_file"])
                    if sharded:
                        kept[fi] = (text, rows)        # this rank's rows of the file, final: they travel as text behind the last file
                    else:
                        out.write(text)
                        total_rows += rows
                st["vcf_s"] += time.perf_counter() - t0

            tev = lambda: torch.cuda.Event(enable_timing=True)
            # h1 is what the main thread waits on before a host set is staged again: a blocking event, so that the wait sleeps (the host
            # threads are the scarce resource of this pipeline: under a 16-core quota the staging + row threads use 13-14 of them)
            ev = [dict(h0=tev(), h1=torch.cuda.Event(enable_timing=True, blocking=True), c0=tev(), c1=tev()) for _ in passes]
            seg_futs, next_seg = [], 0
            with ThreadPoolExecutor(max_workers=1) as pool, ThreadPoolExecutor(max_workers=1) as writer:
                futs = [pool.submit(stage, j) for j in range(min(2, len(passes)))]
                st["setup_s"] += time.perf_counter() - t_begin
                for k, (fi, a, b, o) in enumerate(passes):
                    m = b - a
                    t_w = time.perf_counter()
                    e, t_stage = futs[k].result()
                    t_i = time.perf_counter()
                    st["wait_stage_s"] += t_i - t_w; st["stage_s"] += t_stage
                    st["passes"] += 1; st["passes_int16"] += int(e == 2); st["sites"] += m
                    hs, ds = hsets[k % n_sets], dsets[k % n_sets]
                    nb = m * 594 * e
                    if ds.free is not None:
                        copy_stream.wait_event(ds.free)
                    with torch.cuda.stream(copy_stream):
                        ev[k]["h0"].record(copy_stream)
                        ds.x[:nb].copy_(hs.x[:nb], non_blocking=True)
                        ev[k]["h1"].record(copy_stream)
                    hs.h2d_done = ev[k]["h1"]
                    st["bytes_h2d"] += nb
                    t_c = time.perf_counter()
                    if k + 2 < len(passes):
                        nxt = hsets[(k + 2) % n_sets]
                        if nxt.h2d_done is not None:
                            nxt.h2d_done.synchronize()
                        futs.append(pool.submit(stage, k + 2))
                    t_s = time.perf_counter()
                    main.wait_event(ev[k]["h1"])
                    ev[k]["c0"].record(main)
                    x = ds.x[:nb].view(torch.int16 if e == 2 else torch.int32).view(m, 33, 18)
                    if e == 2:
                        x = x.to(torch.int32)                                         # (1.2 KB read + 2.4 KB written per site: ~1 ns of the forward's 51)
                    # argmax / max of both heads (10 bytes per site) are written by the heads kernel straight into the pinned result arrays:
                    # the H2D copy of a pass is the only copy-engine work of the run
                    if a == 0 and fi >= n_slots and fi - n_slots < len(seg_futs):
                        seg_futs[fi - n_slots].result()                                # the rows of the file that had this result slot are written
                    r = (fi % n_slots) * max_n + a - files[fi]["lo"]
                    ctx.pileup_forward_windows_calls(x.view(m * 33, 18), centers[:m],
                                                     calls_out=(res["ga"][r:r + m], res["za"][r:r + m], res["gm"][r:r + m], res["zm"][r:r + m]))
                    ev[k]["c1"].record(main)
                    ds.free = torch.cuda.Event(blocking=last_pass_of[fi] == k); ds.free.record(main)   # blocking: the writer thread sleeps on it
                    if last_pass_of[fi] == k:
                        while next_seg <= fi:
                            seg_futs.append(writer.submit(rows_of, next_seg, ds.free if next_seg == fi else None)); next_seg += 1
                    t_e = time.perf_counter()
                    st["issue_s"] += t_e - t_i
                    if "trace" in st:
                        st["trace"].append((k, m, t_w, t_i, t_c, t_s, t_e, t_stage))
                t_d = time.perf_counter()
                torch.cuda.synchronize(dev)
                for sf in seg_futs:
                    sf.result()
                st["drain_s"] += time.perf_counter() - t_d
            t_a = time.perf_counter()
            for k, e_ in enumerate(ev):
                st["h2d_s"] += e_["h0"].elapsed_time(e_["h1"]) * 1e-3
                st["gpu_s"] += e_["c0"].elapsed_time(e_["c1"]) * 1e-3
                if k:                                    # compute stream idle between two passes: waiting for a copy or for the host
                    gap = ev[k - 1]["c1"].elapsed_time(e_["c0"]) * 1e-3
                    st["gpu_idle_s"] += gap
                    if "gaps" in st and gap > 5e-4:
                        st["gaps"].append((k, round(gap * 1e3, 2), round(ev[k - 1]["c1"].elapsed_time(e_["h1"]), 2), round(e_["h0"].elapsed_time(e_["h1"]), 2)))
            st["account_s"] += time.perf_counter() - t_a
        if sharded:
            # every rank's rows are final text (whole batches of every file): the sizes travel as one small object, the text in ONE rooted
            # gather; rank 0 puts the pieces in file-major, rank-minor order
            t0 = time.perf_counter()
            mine = [(len(kept[fi][0]), kept[fi][1]) if fi in kept else (0, 0) for fi in range(len(files))]
            sizes = [None] * world
            tdist.all_gather_object(sizes, mine)
            backend_dev = torch.device("cuda", ctx.device) if tdist.get_backend() == "nccl" else "cpu"
            allt = gather_text(b"".join(kept[fi][0] for fi in range(len(files)) if fi in kept), backend_dev)
            if rank == 0:
                start = np.concatenate([[0], np.cumsum([sum(l for l, _ in sz) for sz in sizes])])
                within = [np.concatenate([[0], np.cumsum([l for l, _ in sz])]) for sz in sizes]
                for i in range(len(files)):
                    for r in range(world):
                        out.write(allt[int(start[r] + within[r][i]):int(start[r] + within[r][i + 1])])
                        total_rows += sizes[r][i][1]
            st["gather_s"] = st.get("gather_s", 0.0) + time.perf_counter() - t0
    finally:
        if out:
            out.close()
        for f in files:
            if f["fd"] >= 0:
                os.close(f["fd"])
    return total_rows


predict_pileup_bins.__doc__ = _predict_pileup_bins.__doc__


# ---- a whole-genome mpileup text -> pileup.vcf (DNA_ExtractChrPileupData + everything behind it) ----------------------------------------
class _KeySet:
    """what nsnp_mpileup_tokenise_contigs adds to a _ColSet: the contig index and the key of every line of one chunk"""
    def __init__(self, cap_cols, dev):
        import torch
        self.cid = torch.empty(cap_cols, dtype=torch.int32, device=dev)
        self.key = torch.empty(cap_cols, dtype=torch.int64, device=dev)


def fai_names(fai_text):
    """the contig names of a .fai (its text, or its path as host.vcf_header takes it), in its order"""
    if isinstance(fai_text, os.PathLike) or (isinstance(fai_text, str) and "\n" not in fai_text and "\t" not in fai_text and os.path.isfile(fai_text)):
        with open(fai_text) as f:
            fai_text = f.read()
    return [line.split()[0] for line in fai_text.split("\n") if line.strip()]


def cut_rows_by_contig(keys):
    """keys: int64 [n], the key column of call rows in text order ((contig index << _lib.KEY_SHIFT) | position) -> [(contig index, lo, hi)]:
    the rows of every contig, in the order the contigs appear.  NanoSNPError when a contig's rows come in two pieces."""
    from ._lib import KEY_SHIFT, NanoSNPError
    k = np.asarray(keys, np.int64)
    if not k.size:
        return []
    cid = k >> KEY_SHIFT
    edges = np.flatnonzero(cid[1:] != cid[:-1]) + 1
    lo = np.concatenate([[0], edges]); hi = np.concatenate([edges, [k.size]])
    out = [(int(cid[a]), int(a), int(b)) for a, b in zip(lo, hi)]
    if len({c for c, _, _ in out}) != len(out):
        raise NanoSNPError("call rows: the rows of one contig come in two separate pieces")
    return out


def complete_rows(key):
    """key: column 0 of call rows in text order (a float64 / int64 torch tensor, every contig's rows in one piece) -> how many leading
    rows belong to contigs that are complete when more of the text may follow: all but the trailing rows of the LAST row's contig.  The
    table index says nothing about the order of the text (contigs= may be sorted otherwise than the text is), so the rule looks at
    nothing but where the last row's contig begins."""
    from ._lib import KEY_SHIFT
    n = int(key.shape[0])
    if n == 0:
        return 0
    base = (int(key[-1].item()) >> KEY_SHIFT) << KEY_SHIFT
    mine = (key >= base) & (key < base + (1 << KEY_SHIFT))         # (both bounds are exact in a float64)
    return n - int(mine.sum().item())


class ContigRuns:
    """The run tables of a streamed text's chunks ({first line, contig index} per run: nsnp_mpileup_tokenise_contigs), put together on the
    host: which wanted contigs the text holds, in its order - and the refusal of a wanted contig that comes in two separate runs (the
    reference's splitter would open its file a second time with "w" and keep only the last run)."""
    def __init__(self, names):
        self.names = list(names)
        self.order = []
        self._seen = set()

    def feed(self, runs, n_lines, own_lo, own_hi):
        """runs: int64 [r, 2] of one chunk of n_lines lines of which [own_lo, own_hi) are its own (the others: halo, re-read from its
        neighbours) -> the wanted contigs that START among the own lines, in order"""
        from ._lib import NanoSNPError
        runs = np.asarray(runs, np.int64).reshape(-1, 2)
        started = []
        for i in range(len(runs)):
            first, cid = int(runs[i, 0]), int(runs[i, 1])
            end = int(runs[i + 1, 0]) if i + 1 < len(runs) else int(n_lines)
            if cid < 0 or end <= own_lo or first >= own_hi or first < own_lo:
                continue                                   # (a run that began in front of the own lines was counted by the chunk that owns its first line)
            if cid in self._seen:
                raise NanoSNPError(f"{self.names[cid]}: the text holds this contig in two separate runs (the reference's splitter would keep "
                                   "only the last one)")
            self._seen.add(cid); self.order.append(cid); started.append(cid)
        return started


def _stream_text_dev(model, text, table, chunk_bytes, min_af, min_coverage, stats, on_rows, cap_runs=None, indel_min_af=None, records=None,
                     name_cap=1024, beds=None):
    """_stream_contig_dev for a text of several contigs: the same chunk loop over the same buffer sets (_run_text_chunks, _text_chunk_sets)
    with nsnp_mpileup_tokenise_contigs in the tokeniser's place and its
    `key` where the per-contig path hands a position to the window rule and the call rows.  The run table of every chunk arrives in pinned
    memory with its counts.  on_rows(rows_k, started): the call rows of a chunk ([n, 13] float64 on the device, column 0 = key) or None, and
    the wanted contigs that start among the chunk's own lines; called in chunk order as soon as the chunk's last kernels are issued.
    records (mpileup_to_bins; None: nothing below changes): the tokenise station also compares column 0 of every line with the table name of
    its contig while the chunk's text is still resident (nsnp_mpileup_line_names_contigs), and the third station issues no forward -
    records(k, counts, own centres, _ChunkColumns with the keys as pos, main) is called for every chunk that owns sites; on_rows is not
    called, the wanted contigs the text holds are tracker.order.  indel_min_af (None: min_af) goes to the encode.
    beds (a _lib.BedTable of `table`; None: exactly the launches issued without): with an extended table every chunk's columns pass
    nsnp_pileup_filter_columns_keys in front of the encode, into one of three filter sets - every line tested against the bitmap of its OWN
    contig, the images of the chunk's own range kept on the device for the selection - and the chunk's line_idx is compacted with them: the line
    that emits a site is the 16th KEPT line behind its centre.  With a confident table the encode is nsnp_pileup_encode_columns_keys.  The run
    tables still describe the unfiltered lines: a wanted contig whose lines are all dropped is still held by the text."""
    import time
    import torch
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    finder, arr = _as_bytes_like(text)
    st = _stream_stats(stats)
    t_enter = time.perf_counter()
    tracker = ContigRuns(table.names)
    if not arr.size:
        return tracker
    # the buffer sets of _stream_contig_dev, kept on the model and shared with it (one call at a time per model)
    sets = _text_chunk_sets(model, finder, 0, arr.size, chunk_bytes, dev)
    ranges, csets, main = sets.ranges, sets.csets, sets.main
    ksets = getattr(model, "_key_dev_sets", None)
    if not ksets or len(ksets) < len(csets) or ksets[0].key.device != dev or min(k_.key.numel() for k_ in ksets) < max(c_.pos.numel() for c_ in csets):
        ksets = model._key_dev_sets = [_KeySet(c_.pos.numel(), dev) for c_ in csets]
    # the run table of a chunk: one entry per KB of text, at least 4096 - a run is at least one line, and a chunk whose runs average fewer
    # than ten lines is refused with a status that says so (16 bytes per entry in pinned memory: 1 MB per slot at 64 MB chunks)
    cap_runs = int(cap_runs or max(4096, sets.cap // 1024))
    n_ring = 4                                             # a chunk's counts and run table are read one chunk late: four slots are never in use at once
    if getattr(model, "_run_pin", None) is None or model._run_pin.shape[1] < cap_runs:
        model._run_pin = torch.zeros((n_ring, cap_runs, 2), dtype=torch.int64, pin_memory=True)
        model._ctok_meta_pin = torch.zeros((n_ring, 4), dtype=torch.int64, pin_memory=True)
    meta_pin, tok_pin, run_pin = _count_slots(model, "_meta_pin", len(ranges)), model._ctok_meta_pin, model._run_pin
    started = {}                                           # chunk -> the wanted contigs that start among its own lines
    names_pin = _count_slots(model, "_names_meta_pin", n_ring) if records is not None else None
    names_of = {}
    ext_bed = conf_bed = fsets = fmeta = None
    if beds is not None:
        ext_bed, conf_bed = beds.ext, beds.conf
        if ext_bed is not None:
            fsets = getattr(model, "_filkey_dev_sets", None)
            if not fsets or fsets[0].pos.device != dev or fsets[0].pos.numel() < csets[0].pos.numel() or fsets[0].bases.numel() < csets[0].bases.numel():
                fsets = model._filkey_dev_sets = [_FilKeySet(csets[0].pos.numel(), csets[0].bases.numel(), dev) for _ in range(3)]
                if not sets.fresh:
                    sets.copy_stream.wait_stream(main)     # (new filter sets are new device sets: _text_chunk_sets says why the copy stream waits)
            fmeta = torch.zeros((len(ranges), 4), dtype=torch.int64, device=dev)

    def tokenise(k, text_k, cs):
        ks = ksets[k % len(csets)]
        ctx.mpileup_tokenise_contigs_into(text_k, table, cs.pos, cs.off, cs.bases, cs.ref, ks.cid, ks.key, run_pin[k % n_ring],
                                          tok_pin[k % n_ring], stream=main)
        if records is not None:
            names_of[k] = ctx.mpileup_line_names_contigs(text_k, ks.cid, table, min(int(text_k.numel()) // 10 + 2, int(ks.cid.numel())), name_cap,
                                                         meta=names_pin[k % n_ring], stream=main)[:2]

    def encode(k, cs, n_lo, n_hi):
        M, nb, status, n_runs = tok_pin[k % n_ring].tolist()
        if status & ctx.TOK_EFORMAT:
            raise host.HostError("malformed input (a line with fewer than five tab-separated fields)")
        if status & ctx.TOK_BLANK:
            raise host.HostError("mpileup text holds empty line(s): malformed input (every line must be one pileup column)")
        if status & ctx.TOK_ENAME:
            raise host.HostError("mpileup text holds a contig name longer than 255 bytes")
        if status & ctx.TOK_EPOS:
            raise ValueError("position outside the reference sequence of the line's contig")
        if status & ctx.TOK_ERANGE:
            if n_runs > cap_runs:
                raise host.HostError(f"a chunk of the text holds {n_runs} contig runs, more than the {cap_runs} budgeted (one per KB of text): "
                                     "use a smaller chunk_bytes")
            raise host.HostError(f"a chunk of the text holds {M} lines / {nb} column-5 bytes, more than its column set of {cs.pos.numel()} lines / "
                                 f"{cs.bases.numel()} bytes (lines shorter than 10 bytes: malformed input)")
        if status:
            raise host.HostError(f"tokeniser status {status}")
        started[k] = tracker.feed(run_pin[k % n_ring, :n_runs].numpy(), M, n_lo, M - n_hi)
        own = M - n_lo - n_hi
        st["columns"] += own
        names = None
        if records is not None:
            names = names_of.pop(k)
            n_other, n_status, _, _ = names_pin[k % n_ring].tolist()
            if n_status:
                raise _NamesOverflow(n_other)
            if n_other == 0:
                names = None                                 # (every line names its contig: the records carry the table's names)
        if own <= 0:
            return None
        d_key, d_off, d_bases, d_ref = ksets[k % len(csets)].key[:M], cs.off[:M + 1], cs.bases[:max(nb, 1)], cs.ref[:M]
        if ext_bed is not None:
            # the lines outside the extended BED leave the arrays, the name index of every line with them; where the chunk's own range
            # [n_lo, M - n_hi) lies among the kept columns stays on the device (fmeta[k][2:])
            d_key, d_off, d_bases, d_ref, d_idx, _ = ctx.pileup_filter_columns_keys(d_key, d_off, d_bases, d_ref, table, ext_bed,
                                                                                    aux=None if names is None else names[0], own_lo=n_lo,
                                                                                    own_hi=M - n_hi, meta=fmeta[k],
                                                                                    out=fsets[k % len(fsets)].out, stream=main)
            if names is not None:
                names = (d_idx, names[1])
        if conf_bed is not None:
            counts, depth, flags, _ = ctx.pileup_encode_columns_keys(d_bases, d_off, d_ref, d_key, table, conf_bed, min_af, min_coverage,
                                                                     want_max_del=False, indel_min_af=indel_min_af)
        else:
            counts, depth, flags = ctx.pileup_encode_columns(d_bases, d_off, d_ref, min_af, min_coverage, indel_min_af=indel_min_af)
        if ext_bed is not None:
            center = ctx.pileup_select_sites_range_dev(d_key, flags, fmeta[k][2:], meta_pin[k], stream=main)
        else:
            center = ctx.pileup_select_sites_range(d_key, flags, n_lo, M - n_hi, meta_pin[k], stream=main)
        if records is not None:
            return d_key, counts, center, _ChunkColumns(d_bases, d_off, d_ref, d_key, depth, None, names)
        return d_key, counts, center

    def calls(k, job):
        if records is not None:
            started.pop(k)
            if job is not None:
                _, c_lo, c_hi, _ = meta_pin[k].tolist()
                if c_hi > c_lo:
                    records(k, job[1], job[2][c_lo:c_hi], job[3], main)
            return
        rows_k = None
        if job is not None:
            d_key, counts, center = job
            _, c_lo, c_hi, _ = meta_pin[k].tolist()
            if c_hi > c_lo:
                centers = center[c_lo:c_hi]
                gt, zy, ga, za, gm, zm = ctx.pileup_forward_windows_calls(counts, centers)
                rows_k = ctx.pileup_call_rows(counts, centers, d_key, ga, za, gm, zm)
        on_rows(rows_k, started.pop(k))

    st["setup_s"] += time.perf_counter() - t_enter
    finalize = _run_text_chunks(sets, arr, st, tokenise, encode, calls)
    done = torch.cuda.Event(); done.record(main)
    finalize(done)
    return tracker


def _format_key_rows(rows, table, batch_size, score_mode, ctx, nthreads=None):
    """call rows whose column 0 is a key, of any number of WHOLE contigs in text order -> [(VCF text, rows written)] per contig: the rows
    come to the host as typed columns (pileup_rows_unpack writes them into pinned memory), are cut by contig from the key's high bits
    (cut_rows_by_contig) and formatted with the reference's batches restarting at every contig, as its loop restarts them with every
    .bin file"""
    import torch
    from ._lib import KEY_SHIFT
    n = int(rows.shape[0])
    hb = getattr(ctx, "_rows_host", None)
    if hb is None or hb[0].numel() < n:
        cap = max(n + n // 4, 65536)
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
        hb = ctx._rows_host = (mk(cap, torch.int64), mk(cap, torch.uint8), mk(cap, torch.uint8), mk(cap, torch.float32), mk(cap, torch.float32),
                               mk((cap, 8), torch.float32))
    s_ = torch.cuda.current_stream(rows.device)
    ctx.pileup_rows_unpack(rows.contiguous(), hb, stream=s_)
    # the reference base of every site: one gather from the resident genome
    key = rows[:, 0].to(torch.int64)
    refb = table.genome[table.seq_off[key >> KEY_SHIFT] + (key & ((1 << KEY_SHIFT) - 1)) - 1].cpu()
    s_.synchronize()
    keys, ga, za, gm, zm = (t[:n].numpy() for t in hb[:5])
    cov = hb[5][:n].numpy()
    site_ref = refb.numpy() & 0xDF                                           # make_predict_data/main.cpp:91 upper-cases
    out = []
    for cid, a, b in cut_rows_by_contig(keys):
        pos = keys[a:b] & ((1 << KEY_SHIFT) - 1)
        out.append(host.vcf_format_batches(host.ContigTable([table.names[cid]]), np.zeros(b - a, np.int32), pos, site_ref[a:b], ga[a:b], za[a:b],
                                           gm[a:b], zm[a:b], cov[a:b], batch_size=batch_size, score_mode=score_mode, nthreads=nthreads))
    return out


def call_mpileup(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, contigs=None, batch_size=1000, score_mode=host.SCORE_FLOAT64,
                 chunk_bytes=64 << 20, min_af=0.12, min_coverage=6, stats=None, extended_bed=None, confident_bed=None):
    """call_variants from the file the reference's stage 1 starts from: ONE mpileup text holding every contig (samtools mpileup BAM -o
    pileup_data, make_predict_data.sh:117,151), not cut into <chr>.mpileup files by DNA_ExtractChrPileupData first.  mpileup_path_or_bytes:
    a path, or bytes / mmap / uint8 array; contigs: the wanted names (the reference's ALL_CHR_LIST; None: every name of fai_text, as -g);
    writes pileup.vcf, returns the rows written.
    The text is ONE stream (_stream_text_dev): staged chunks of whole lines with the 16-line halo cross PCIe once, the device finds the contig
    of every line (nsnp_mpileup_tokenise_contigs: the host never scans the text for names) and hands encode, window rule and call rows
    a key = (contig index << 36) | position, so that no window crosses a contig; lines of names outside `contigs` become filler the
    window rule makes nothing of.  The rows of finished contigs are cut by contig on the host from the key's high bits and formatted - the
    batches restart with every contig - and written, in the order the contigs appear in the text, on a writer thread while the text
    streams on.  For a text whose wanted contigs each form one run the file equals, byte for byte, call_variants over the files the
    splitter would have written, at every chunk_bytes and whatever the order of `contigs` (the table) is against the order of the text.  The wanted contigs' sequences are resident on the device (3.1 GB for a human genome).
    Departures from the splitter: a wanted contig in two separate runs raises NanoSNPError (the splitter would reopen its file with "w" and
    keep only the last run); an empty line is refused as the tokeniser refuses it (the splitter skips it).  NotImplementedError: under a
    process group of more than one rank, with NSNP_TOKENISE=host, with extended_bed= / confident_bed=."""
    if extended_bed is not None or confident_bed is not None:
        raise NotImplementedError("call_mpileup: BED region filters over several contigs (call_mpileup_bed takes them)")
    return _call_mpileup(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, None, None, contigs=contigs, batch_size=batch_size,
                         score_mode=score_mode, chunk_bytes=chunk_bytes, min_af=min_af, min_coverage=min_coverage, stats=stats)


def call_mpileup_bed(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, *, extended_bed=None, confident_bed=None, **kw):
    """call_mpileup with the reference's two region filters (-extended_confident_bed / -confident_bed, make_candidate_snp_tensor/main.cpp:
    158-201) over ALL contigs of the text: each a path - checked against the whole index fai_text, as the reference reads it - or {contig:
    intervals}.  A line is read at all only where the extended BED has the bit of its position in its OWN contig; a column is a candidate only
    where the confident BED has a bit in [p - 1, p + max_del_length + 1) of its own contig (bed.py; a reach past a contig's end never sees the
    next contig's bits).  For a text whose wanted contigs each form one run the file equals, byte for byte, call_variants(..., extended_bed=,
    confident_bed=) over the files the splitter would have written, at every chunk_bytes with ascending positions.  The bitmaps are resident
    beside the sequences (_lib.BedTable: 1 bit per base of every contig a BED mentions).  **kw and the refusals: as call_mpileup (a process
    group of more than one rank, NSNP_TOKENISE=host); with both BEDs None this IS call_mpileup, launch for launch."""
    return _call_mpileup(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, extended_bed, confident_bed, **kw)


def call_mpileup_groups(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, *, quality_threshold=19.0, adjacent_size=5,
                        support_quality=14.0, reference_bug=False, nthreads=10, extended_bed=None, confident_bed=None, **kw):
    """call_mpileup_bed that also selects the stage-4 site groups (merge.select_groups: every low-quality site with its adjacent_size nearest
    confident heterozygous neighbours on each side) from the call rows while they are still on the device, instead of from the pileup.vcf
    they become: -> (rows written, merge.DeviceGroups).  The file is call_mpileup_bed's, byte for byte.  The rows of every hand-over of
    complete contigs go through nsnp_pileup_select_groups (merge.select_groups_rows) on the writer thread's stream behind their formatting;
    the pieces are put together when the text is over, `rows` of the DeviceGroups counting the call rows of the whole run in text order.
    groups.to_lists() equals merge.select_groups on the file with the same thresholds, nthreads and reference_bug (False here by default:
    every contig is kept).  **kw and the refusals: as call_mpileup_bed; also NanoSNPError for positions that do not ascend strictly inside
    a contig (select_groups would keep the last row of a repeated position)."""
    import torch
    from . import merge
    from ._lib import KEY_SHIFT
    batch_size, score_mode = kw.get("batch_size", 1000), kw.get("score_mode", host.SCORE_FLOAT64)
    parts, offsets = [], [0]

    def on_contigs(rows, table, ctx):
        key = rows[:, 0].to(torch.int64)
        ref_base = table.genome[table.seq_off[key >> KEY_SHIFT] + (key & ((1 << KEY_SHIFT) - 1)) - 1]
        parts.append(merge.select_groups_rows(ctx, rows, ref_base, table.names, quality_threshold=quality_threshold, adjacent_size=adjacent_size,
                                              support_quality=support_quality, batch_size=batch_size, score_mode=score_mode, reference_bug=False))
        offsets.append(offsets[-1] + int(rows.shape[0]))

    n_rows = _call_mpileup(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, extended_bed, confident_bed, on_contigs=on_contigs, **kw)
    if not parts:
        dev = torch.device("cuda", model.ctx.device)
        return n_rows, merge.DeviceGroups.empty(kw.get("contigs") or fai_names(fai_text), adjacent_size, dev, score_mode)
    return n_rows, merge.DeviceGroups.concat(parts, offsets[:-1], nthreads, reference_bug)


def _call_mpileup(model, mpileup_path_or_bytes, fasta_path, fai_text, output_file, extended_bed, confident_bed, contigs=None, batch_size=1000,
                  score_mode=host.SCORE_FLOAT64, chunk_bytes=64 << 20, min_af=0.12, min_coverage=6, stats=None, on_contigs=None):
    """the one body of call_mpileup, call_mpileup_bed and call_mpileup_groups.  on_contigs(rows, table, ctx) (None: nothing below changes):
    called on the writer thread, under its stream and with its context, with the call rows of every hand-over of complete contigs - in
    text order, behind their formatting and before they are released"""
    import time
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    import torch
    import torch.distributed as tdist
    from . import _lib
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("call_mpileup: sharding a whole-genome text over ranks")
    if tokenise_mode() != "device":
        raise NotImplementedError("call_mpileup: the contigs are found by the device tokeniser (NSNP_TOKENISE=host is not supported)")
    if not torch.cuda.is_available():
        raise _lib.NanoSNPError("no GPU visible: nanosnp_amd has no CPU fallback")
    names = list(contigs) if contigs is not None else fai_names(fai_text)
    table = _lib.ContigTable(fasta=fasta_path, names=names, device=model.ctx.device)
    beds = None if extended_bed is None and confident_bed is None else _lib.BedTable(table, extended_bed, confident_bed, fai_text)
    st = stats if stats is not None else {}
    dev = torch.device("cuda", model.ctx.device)
    side = getattr(model, "_rows_stream", None)
    if side is None:
        side = model._rows_stream = torch.cuda.Stream(dev)
        model._rows_ctx = _lib.Context(model.ctx.device)     # the writer thread's own context (call_contigs)
    wctx = model._rows_ctx
    few = max(1, host.lib().nsnp_host_threads() // 4)
    n_rows = 0
    with _text_of(mpileup_path_or_bytes) as src, open(output_file, "wb") as f:
        f.write(host.vcf_header(fai_text).encode())
        acc, futs, carry = [], deque(), []

        def finish(pieces, done, last):
            """writer thread (one worker: the hand-overs run in the order they were made): formats and writes the rows of the contigs that
            are complete - every one but the contig of the last row, whose rows may go on in later chunks and wait in `carry` for the
            next hand-over - or everything when the text is over.  Returns the rows written."""
            done.synchronize()
            t0 = time.perf_counter()
            pieces = carry + pieces
            del carry[:]
            if not pieces:
                return 0
            with torch.cuda.stream(side):
                rows = torch.cat(pieces) if len(pieces) > 1 else pieces[0]
                if not last:
                    keep = complete_rows(rows[:, 0])
                    if keep < rows.shape[0]:
                        carry.append(rows[keep:])
                    rows = rows[:keep]
                parts = _format_key_rows(rows, table, batch_size, score_mode, wctx, nthreads=0 if last else few) if rows.shape[0] else []
                if on_contigs is not None and rows.shape[0]:
                    on_contigs(rows, table, wctx)
            nr = 0
            for t_, r_ in parts:
                f.write(t_); nr += r_
            st["vcf_s"] = st.get("vcf_s", 0.0) + time.perf_counter() - t0
            return nr

        with host.gc_paused(), ThreadPoolExecutor(max_workers=1) as writer:
            main = torch.cuda.current_stream(dev)

            def flush(last):
                """hands the rows issued so far to the writer; the issuing thread waits only when two hand-overs are still unfinished (the
                rows they hold stay allocated on the device until they are written)"""
                nonlocal acc, n_rows
                while len(futs) > 1:
                    n_rows += futs.popleft().result()
                if acc or last:
                    done = torch.cuda.Event(); done.record(main)
                    futs.append(writer.submit(finish, acc, done, last))
                    acc = []

            def on_rows(rows_k, started):
                if started and acc:
                    flush(False)                             # a wanted contig begins in this chunk: the ones in front of it are complete
                if rows_k is not None:
                    st["sites"] = st.get("sites", 0) + int(rows_k.shape[0])
                    acc.append(rows_k)

            try:
                _stream_text_dev(model, src, table, chunk_bytes, min_af, min_coverage, st, on_rows, beds=beds)
                flush(True)
                while futs:
                    n_rows += futs.popleft().result()
            except BaseException:
                for fu in futs:                              # (what the writer has begun it finishes: the executor waits for it)
                    fu.cancel()
                raise
        st["vcf_rows"] = st.get("vcf_rows", 0) + n_rows
        return n_rows


# ---- <chr>.mpileup text -> <chr>.pd.bin: stage s1 alone (make_predict_data.sh:167-234) ------------------------------------------------
class _RecSlot:
    """pinned result buffers of one chunk's records in flight: written by the record kernels, read by the writer thread"""
    def __init__(self, rows, blob_bytes):
        import torch
        from ._lib import Context
        self.rows = int(rows)
        self.matrix = torch.empty(self.rows * 594 * 4, dtype=torch.uint8, pin_memory=True)          # (room for int32: a restart keeps the slot)
        self.position = torch.empty((self.rows, Context.POSITION_WIDTH), dtype=torch.uint8, pin_memory=True)
        self.blob = torch.empty(int(blob_bytes), dtype=torch.uint8, pin_memory=True)
        self.offsets = torch.empty(self.rows + 1, dtype=torch.int64, pin_memory=True)
        self.site_key = torch.empty(max(self.rows, 1), dtype=torch.int64, pin_memory=True)          # (mpileup_to_bins: the key of every site)
        self.meta = torch.zeros((2, 4), dtype=torch.int64, pin_memory=True)                         # window_records' and alt_info's
        self.busy = None                                                                           # the writer thread's future over this slot

    def matrix_as(self, elem):
        import torch
        return self.matrix.view(torch.int16 if elem == 2 else torch.int32)[:self.rows * 594]


def _bins_refusals():
    """what the stage-1 entries do not do, said before anything is touched"""
    import torch
    import torch.distributed as tdist
    from ._lib import NanoSNPError
    if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        raise NotImplementedError("contig_to_bin / make_pileup_bins under a process group of more than one rank (window files are not sharded)")
    if tokenise_mode() == "host":
        raise NotImplementedError("contig_to_bin / make_pileup_bins with NSNP_TOKENISE=host (the records are built from the device tokeniser's columns)")
    if not torch.cuda.is_available():
        raise NanoSNPError("no GPU visible: nanosnp_amd has no CPU fallback")


def _check_matrix_dtype(matrix_dtype):
    from . import sitefile
    if matrix_dtype not in ("int16", "int32"):
        raise sitefile.SiteFileError("matrix_dtype: 'int16' or 'int32'")


def _position_name(contig):
    """a contig name (str or bytes) -> the bytes a position string begins with; ValueError for one the position field has no room for"""
    from . import sitefile
    name = contig.encode() if isinstance(contig, str) else bytes(contig)
    if not name or b"\0" in name or len(name) + 1 + 11 + 1 + 33 > sitefile.POSITION_WIDTH:
        raise ValueError(f"{contig!r}: a contig name of 1 to {sitefile.POSITION_WIDTH - 46} bytes without NUL is needed for the "
                         f"{sitefile.POSITION_WIDTH}-byte position field")
    return name


def _run_passes(sink, matrix_dtype, run_pass, st, finish):
    """The restart loop of the window writers: run_pass(state) streams the text once into `sink` -> (run again?, result); state = {elem,
    blob_min, name_cap} says how the next pass differs (_records_pass).  Every pass but the last is dropped whole (sink.restart);
    -> finish(the last pass's result); on any error sink.abort() before it leaves."""
    state = dict(elem=2 if matrix_dtype == "int16" else 4, blob_min=0, name_cap=1024)
    try:
        while True:
            again, result = run_pass(state)
            if not again:
                return finish(result)
            st["restarts"] = st.get("restarts", 0) + 1
            sink.restart("int16" if state["elem"] == 2 else "int32")
    except BaseException:
        sink.abort()
        raise


def contig_to_bin(model, mpileup_text, contig, chr_seq, path, *, alt_info=True, matrix_dtype="int16", min_af=0.12, indel_min_af=None,
                  min_coverage=6, chunk_bytes=64 << 20, stats=None, extended_bed=None, confident_bed=None, fai=None):
    """Stage s1 alone: one contig's samtools-mpileup text -> its <chr>.pd.bin (sitefile: position_matrix, position, alt_info,
    alt_info_offsets), the file DNA_CreateCanSnpTensor -> DNA_CreatePredictData -> make_bin_predict_data.py leave behind
    (make_predict_data.sh:167-234), byte for byte what sitefile.pd_to_bin makes of the reference's .pd.  Returns the number of sites.

    model: only the holder of the context and the buffer sets - pileup_model.LSTMNetwork() without weights will do.  The text runs through
    the chunk loop of call_contig (tokenise k, BED filter + encode + select k - 1); where that loop runs the forward, this one issues
    nsnp_pileup_window_records and nsnp_pileup_alt_info for the chunk's own sites into one of three pinned slots, and a writer thread
    appends the slot to a sitefile.PileupBinWriter when its event has passed.  A slot with too few rows is replaced before the launch
    (the site count is on the host by then); a chunk whose alt_info text outgrows its slot, or a count outside int16, starts the contig
    over with larger slots / as int32 - nothing is ever cut.  min_af / indel_min_af / min_coverage, extended_bed / confident_bed / fai: as
    for call_contig; text the reference's reader aborts on raises the same errors.  On any error neither `path` nor `path + ".tmp"` is
    left by this call (a file that was at `path` before stays as it was).
    matrix_dtype: as for sitefile.write_pileup_bin; alt_info=False leaves the two alt_info arrays out.
    The name in a position string is column 0 of the line that emits the site (the line at centre + 16), as the reference prints it:
    `contig` in any text samtools or the splitter wrote; a line with another token there has that token (nsnp_mpileup_line_names).  Not
    together with an extended BED (NotImplementedError when such a line is met), and a token longer than 37 bytes is refused.
    NOT done here: one whole-genome text (mpileup_to_bins does that), sharding over a process group, a .pd TEXT writer, the reference's
    .tensor / .alt_info side files."""
    from concurrent.futures import ThreadPoolExecutor
    from . import sitefile
    _bins_refusals()
    name = _position_name(contig)
    _check_matrix_dtype(matrix_dtype)
    beds = _contig_beds(extended_bed, confident_bed, contig, chr_seq, fai)
    st = _stream_stats(stats)
    writer = sitefile.PileupBinWriter(path, matrix_dtype, alt_info)
    source = _ContigRecords(model.ctx, name, contig, chr_seq, beds, writer, alt_info)
    with ThreadPoolExecutor(max_workers=1) as pool:
        n = _run_passes(writer, matrix_dtype, lambda state: _records_pass(model, source, mpileup_text, chunk_bytes, min_af, indel_min_af, min_coverage,
                                                                          st, state, pool), st, lambda _: writer.close())
    st["sites"] = st.get("sites", 0) + n
    return n


def _records_pass(model, source, text, chunk_bytes, min_af, indel_min_af, min_coverage, st, state, pool):
    """One pass of contig_to_bin / mpileup_to_bins / mpileup_to_train_bins over the text -> (True when it has to be run again - state says how:
    elem 4, blob_min bytes per slot, or name_cap entries per name table -, what source.stream returned).
    source (_ContigRecords / _KeyedRecords) says how the text is streamed, which two record kernels fill a slot, where a finished slot is
    appended and how a refusal reads; the three pinned slots taken in turn, the writer thread's pieces and the restart decisions are here."""
    import torch
    from ._lib import NanoSNPError
    ctx, alt_info, elem = source.ctx, source.alt_info, state["elem"]
    text_len = int(_as_bytes_like(text)[1].size)
    slots = getattr(model, source.slots_attr, None)
    if slots is None:
        slots = [None, None, None]
        setattr(model, source.slots_attr, slots)
    flag = dict(overflow=False, alt_need=0, status=0)
    turn, spans = [0], []

    def write_piece(slot, n, done):
        done.synchronize()
        m = slot.meta.numpy()
        if m[0, 1]:
            flag["overflow"] = True
        if m[0, 2]:
            flag["status"] = int(m[0, 2])
        if source.label_status(slot):
            flag["status"] = flag["status"] or 1
        if alt_info and (m[1, 1] & ctx.TOK_ERANGE):
            flag["alt_need"] = max(flag["alt_need"], int(m[1, 0]))
        if alt_info and (m[1, 1] & ~ctx.TOK_ERANGE):         # (a key outside the table: only nsnp_pileup_alt_info_keys reports another bit)
            flag["status"] = int(m[1, 1])
        if flag["overflow"] or flag["alt_need"] or flag["status"]:
            return                                           # (the pass is run again, or refused: nothing more is appended)
        x = slot.matrix.numpy().view(np.int16 if elem == 2 else np.int32)[:n * 594].reshape(n, 33, 18)
        source.append(slot, n, x, int(m[1, 0]))
        st["record_bytes"] = st.get("record_bytes", 0) + n * (594 * elem + 83 + source.label_bytes) + (int(m[1, 0]) + 8 * n if alt_info else 0)

    def records(k, counts, centers, cols, main):
        if flag["overflow"] or flag["alt_need"] or flag["status"]:
            return                                           # (this pass is lost: the rest of it only has to end)
        n = int(centers.shape[0])
        i = turn[0] % 3
        turn[0] += 1
        slot = slots[i]
        if slot is not None and slot.busy is not None:
            slot.busy.result()                               # the writer is done with the slot's previous chunk (three chunks back)
            slot.busy = None
        want_blob = max(64 * n + (1 << 16), state["blob_min"])
        if slot is None or slot.rows < n or slot.blob.numel() < want_blob:
            # (a 30x chunk selects 3-4 % of its columns and budgets one column per 24 bytes: 1 / 64 of them is about as many rows as it fills)
            rows = max(n + n // 4, _cols_for(min(int(chunk_bytes), text_len)) // 64, 1024 if slot is None else slot.rows)
            slot = slots[i] = source.new_slot(rows, max(64 * rows + (1 << 16), state["blob_min"]), main)
        centers = source.label(slot, centers, cols, main, st, flag)
        if centers is None:
            return                                           # (no site of the chunk is kept, or a status that ends the pass)
        n = int(centers.shape[0])
        timed = st.get("time_records")                       # (stats["time_records"] = True: HIP-event time of the record kernels -> stats["window_records_s"], ["alt_info_s"])
        if timed:
            t0, t1, t2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            t0.record(main)
        source.window_records(slot, counts, centers, cols, elem, main)
        if timed:
            t1.record(main)
        if alt_info:
            source.alt_records(slot, centers, cols, main)
        if timed:
            t2.record(main)
            spans.append((t0, t1, t2))
        done = torch.cuda.Event(); done.record(main)
        slot.busy = pool.submit(write_piece, slot, n, done)

    def drain(swallow):
        for slot in slots:
            if slot is not None and slot.busy is not None:
                busy, slot.busy = slot.busy, None
                try:
                    busy.result()
                except BaseException:
                    if not swallow:
                        raise

    try:
        with host.gc_paused():
            result = source.stream(model, text, chunk_bytes, min_af, indel_min_af, min_coverage, st, records, state["name_cap"])
        drain(False)
        for t0, t1, t2 in spans:
            st["window_records_s"] = st.get("window_records_s", 0.0) + t0.elapsed_time(t1) * 1e-3
            st["alt_info_s"] = st.get("alt_info_s", 0.0) + t1.elapsed_time(t2) * 1e-3
            st["record_chunks"] = st.get("record_chunks", 0) + 1
    except _NamesOverflow as e:
        drain(True)
        state["name_cap"] = 2 * e.need + 64
        return True, None
    except BaseException:
        drain(True)                                          # (the streams have been waited for: the writer's pieces end at once)
        raise
    if flag["status"]:
        raise NanoSNPError(source.status_text(flag["status"]))
    if flag["overflow"]:
        if elem == 4:
            raise NanoSNPError(source.overflow_text)
        state["elem"] = 4
        return True, None
    if flag["alt_need"]:
        state["blob_min"] = 2 * flag["alt_need"]
        return True, None
    return False, result


class _ContigRecords:
    """What _records_pass asks of contig_to_bin: one contig's text through _stream_contig_dev, the record kernels that take the contig's one
    name and sequence, every finished slot straight into the one PileupBinWriter.  Nothing of a chunk is labelled or dropped."""
    slots_attr = "_rec_slots"
    label_bytes = 0

    def __init__(self, ctx, name, contig, chr_seq, beds, writer, alt_info):
        self.ctx, self.name, self.contig, self.chr_seq, self.beds, self.writer, self.alt_info = ctx, name, contig, chr_seq, beds, writer, alt_info
        self.overflow_text = f"{contig}: int16 overflow reported for int32 records"

    def status_text(self, status):
        return f"{self.contig}: a selected site outside the columns or the contig (record status {status})"

    def stream(self, model, text, chunk_bytes, min_af, indel_min_af, min_coverage, st, records, name_cap):
        _stream_contig_dev(model, text, self.contig, self.chr_seq, 0, None, chunk_bytes, min_af, min_coverage, st, None, beds=self.beds,
                           indel_min_af=indel_min_af, records=records, name_cap=name_cap)

    def new_slot(self, rows, blob_bytes, main):
        return _RecSlot(rows, blob_bytes)

    def label(self, slot, centers, cols, main, st, flag):
        return centers

    def label_status(self, slot):
        return 0

    def window_records(self, slot, counts, centers, cols, elem, main):
        self.ctx.pileup_window_records(counts, centers, cols.pos, cols.seq, self.name, elem, position_matrix=slot.matrix_as(elem), position=slot.position,
                                       meta=slot.meta[0], stream=main, line_names=cols.names)

    def alt_records(self, slot, centers, cols, main):
        self.ctx.pileup_alt_info(cols.bases, cols.off, cols.ref, cols.pos, cols.depth, centers, cols.seq, blob=slot.blob, offsets=slot.offsets,
                                 meta=slot.meta[1], stream=main)

    def append(self, slot, n, x, blob_bytes):
        if self.alt_info:
            self.writer.append(x, slot.position.numpy()[:n], slot.blob.numpy()[:blob_bytes], slot.offsets.numpy()[:n + 1])
        else:
            self.writer.append(x, slot.position.numpy()[:n])


def make_pileup_bins(model, contigs, fasta_path, fai_text, out_dir, **kw):
    """The s1 drop-in beside call_variants.  contigs: iterable of (name, path to <name>.mpileup), as call_variants takes them; writes
    <out_dir>/<name>.pd.bin per contig (contig_to_bin: its keyword arguments pass through; extended_bed= / confident_bed= are checked
    against fai_text) -> {name: sites}.  The files are what predict_pileup_bins reads."""
    _bins_refusals()
    if kw.get("extended_bed") is not None or kw.get("confident_bed") is not None:
        kw.setdefault("fai", fai_text)
        if not all(b is None or isinstance(b, dict) for b in (kw.get("extended_bed"), kw.get("confident_bed"))):
            from . import bed as _bed                          # (a BED path: parsed once, against the whole index)
            kw["extended_bed"], kw["confident_bed"] = (b if b is None or isinstance(b, dict) else _bed.load_bed(b, kw["fai"])
                                                       for b in (kw.get("extended_bed"), kw.get("confident_bed")))
    os.makedirs(out_dir, exist_ok=True)
    out = {}
    for name, path in contigs:
        seq = host.fasta_load_contig(fasta_path, name)
        with _mapped(path) as text:
            out[name] = contig_to_bin(model, text, name, seq, os.path.join(out_dir, f"{name}.pd.bin"), **kw)
    return out


# ---- one whole-genome mpileup text -> every <chr>.pd.bin (make_predict_data.sh:117-234 without the splitter's pass) ------------------------
def cut_records_by_contig(site_key, alt_offsets=None):
    """The records of one chunk, cut by contig.  site_key: int64 [n], the key of every site in line order ((contig index << _lib.KEY_SHIFT) |
    position: nsnp_pileup_window_records_keys); alt_offsets: int64 [n + 1] into the chunk's alt_info blob, or None
    -> [(contig index, lo, hi, blob_lo, blob_hi, offsets)] in the order the contigs appear: rows [lo, hi), their texts blob[blob_lo:blob_hi]
    and offsets int64 [hi - lo + 1] REBASED to start at 0 (blob_lo = blob_hi = 0 and offsets None without alt_offsets).  A contig that ends
    exactly at the chunk's last site is simply the last piece.  NanoSNPError when a contig's rows come in two pieces."""
    from ._lib import KEY_SHIFT, NanoSNPError
    k = np.asarray(site_key, np.int64).reshape(-1)
    if not k.size:
        return []
    offs = None if alt_offsets is None else np.asarray(alt_offsets, np.int64).reshape(-1)
    if offs is not None and offs.size != k.size + 1:
        raise NanoSNPError("records: alt_offsets must hold one more entry than site_key")
    cid = k >> KEY_SHIFT
    edges = np.flatnonzero(cid[1:] != cid[:-1]) + 1
    lo = np.concatenate([[0], edges]); hi = np.concatenate([edges, [k.size]])
    out = []
    for a, b in zip(lo.tolist(), hi.tolist()):
        if offs is None:
            out.append((int(cid[a]), a, b, 0, 0, None))
        else:
            out.append((int(cid[a]), a, b, int(offs[a]), int(offs[b]), offs[a:b + 1] - offs[a]))
    if len({c for c, *_ in out}) != len(out):
        raise NanoSNPError("records: the sites of one contig come in two separate pieces")
    return out


class _BinStaging:
    """The window files of one mpileup_to_bins call while they are written: every contig's sitefile.PileupBinWriter writes to a staging name
    inside out_dir, and commit() renames the finished files to <out_dir>/<name>.pd.bin only after the whole text has ended without error;
    abort() leaves neither a staging nor a .tmp file of this call, and whatever was in out_dir before stays as it was.  The pieces of a
    contig arrive one after another (a contig is one run of the text), so one writer is open at a time."""

    def __init__(self, out_dir, names, matrix_dtype="int16", alt_info=True):
        import uuid
        self.out_dir, self.names, self.matrix_dtype, self.alt_info = out_dir, list(names), matrix_dtype, bool(alt_info)
        self.tag = f".nsnp-staging-{os.getpid()}-{uuid.uuid4().hex[:12]}"
        self.cur = self.cur_cid = None
        self.done = {}                                       # contig index -> sites, of the staging files that are complete

    suffix = ".pd.bin"

    def staging_path(self, cid):
        return os.path.join(self.out_dir, f"{self.tag}.{int(cid)}")

    def _writer(self, cid):
        from . import sitefile
        return sitefile.PileupBinWriter(self.staging_path(cid), self.matrix_dtype, self.alt_info)

    def _finish(self):
        if self.cur is not None:
            cur, self.cur = self.cur, None
            self.done[self.cur_cid] = cur.close()            # (close() removes its .tmp itself when it fails)

    def append(self, cid, x, position, blob=None, offsets=None):
        """the next piece of contig `cid`, as PileupBinWriter.append takes it"""
        from ._lib import NanoSNPError
        if self.cur is None or self.cur_cid != cid:
            self._finish()
            if cid in self.done or not 0 <= cid < len(self.names):
                raise NanoSNPError(f"records: contig index {cid} outside the table or in two separate pieces")
            self.cur_cid, self.cur = cid, self._writer(cid)
        if self.alt_info:
            self.cur.append(x, position, blob, offsets)
        else:
            self.cur.append(x, position)

    def restart(self, matrix_dtype=None):
        """drops everything written so far: the text is streamed again"""
        self.abort()
        self.matrix_dtype = matrix_dtype or self.matrix_dtype

    def commit(self, order):
        """order: the wanted contigs the text holds, in its order (ContigRuns.order) - one without sites gets its empty file here.
        -> {name: sites}; the files are in place."""
        from ._lib import NanoSNPError
        self._finish()
        if set(self.done) - set(order):
            raise NanoSNPError("records: sites of a contig the text's runs do not hold")
        for cid in order:
            if cid not in self.done:
                self.done[cid] = self._writer(cid).close()
        out = {}
        for cid in order:
            os.replace(self.staging_path(cid), os.path.join(self.out_dir, f"{self.names[cid]}{self.suffix}"))
            out[self.names[cid]] = self.done.pop(cid)
        return out

    def abort(self):
        if self.cur is not None:
            cur, self.cur = self.cur, None
            cur.abort()
        for cid in list(self.done):
            try:
                os.remove(self.staging_path(cid))
            except OSError:
                pass
        self.done = {}


def _staged_bins(out_dir, names, matrix_dtype, alt_info, run_pass, st, staging_cls=None):
    """The file side of mpileup_to_bins: run_pass(staging, state) streams the text once, appending to `staging` -> (run again?, the wanted
    contigs the text holds in its order); state = {elem, blob_min, name_cap} says how the next pass differs.  Every pass but the last is
    dropped whole; the files are renamed into place when the last one has ended, and on any error nothing of this call is left in out_dir
    (out_dir itself neither, when this call made it).  -> {name: sites}"""
    made = not os.path.isdir(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    staging = (staging_cls or _BinStaging)(out_dir, names, matrix_dtype, alt_info)
    try:
        return _run_passes(staging, matrix_dtype, lambda state: run_pass(staging, state), st, staging.commit)
    except BaseException:
        if made:
            try:
                os.rmdir(out_dir)
            except OSError:
                pass
        raise


class _KeyedRecords:
    """What _records_pass asks of mpileup_to_bins: the whole text through _stream_text_dev (-> the wanted contigs it holds, in its order),
    the record kernels that take names and bases out of the resident contig table and hand back every site's key, every finished slot cut
    by contig into the staging.
    train (a _TrainLabels of mpileup_to_train_bins; None: exactly the launches issued without): its slots carry the label rows, its
    label() runs in front of the record kernels and says which centres they get, and the staging gets the label rows and the site keys of
    every piece."""

    def __init__(self, ctx, table, beds, staging, alt_info, train=None):
        self.ctx, self.table, self.beds, self.staging, self.alt_info, self.train = ctx, table, beds, staging, alt_info, train
        self.slots_attr = "_rec_slots" if train is None else "_train_slots"
        self.label_bytes = 0 if train is None else 360
        self.overflow_text = "int16 overflow reported for int32 records"

    def status_text(self, status):
        return ("a selected site outside the columns or its contig, " + ("" if self.train is None else "at a reference byte other than A/C/G/T, ")
                + f"or a name longer than 37 bytes in column 0 (record status {status})")

    def stream(self, model, text, chunk_bytes, min_af, indel_min_af, min_coverage, st, records, name_cap):
        tracker = _stream_text_dev(model, text, self.table, chunk_bytes, min_af, min_coverage, st, None, indel_min_af=indel_min_af, records=records,
                                   name_cap=name_cap, beds=self.beds)
        return list(tracker.order)

    def new_slot(self, rows, blob_bytes, main):
        return _RecSlot(rows, blob_bytes) if self.train is None else self.train.new_slot(rows, blob_bytes, main)

    def label(self, slot, centers, cols, main, st, flag):
        return centers if self.train is None else self.train.label(slot, centers, cols, main, st, flag)

    def label_status(self, slot):
        return self.train is not None and int(slot.lmeta[3])

    def window_records(self, slot, counts, centers, cols, elem, main):
        self.ctx.pileup_window_records_keys(counts, centers, cols.pos, self.table, elem, position_matrix=slot.matrix_as(elem), position=slot.position,
                                            site_key=slot.site_key, meta=slot.meta[0], stream=main, line_names=cols.names)

    def alt_records(self, slot, centers, cols, main):
        self.ctx.pileup_alt_info_keys(cols.bases, cols.off, cols.ref, cols.pos, cols.depth, centers, self.table, blob=slot.blob, offsets=slot.offsets,
                                      meta=slot.meta[1], stream=main)

    def append(self, slot, n, x, blob_bytes):
        alt_info, position, blob = self.alt_info, slot.position.numpy(), slot.blob.numpy()
        # the rows are ascending in line order: every contig of the chunk is one piece
        keys = slot.site_key.numpy()
        for cid, a, b, b_lo, b_hi, offs in cut_records_by_contig(keys[:n], slot.offsets.numpy()[:n + 1] if alt_info else None):
            if self.train is None:
                self.staging.append(cid, x[a:b], position[a:b], blob[b_lo:b_hi] if alt_info else None, offs)
            else:
                self.staging.append(cid, x[a:b], position[a:b], slot.label.numpy()[a:b], blob[b_lo:b_hi] if alt_info else None, offs, keys=keys[a:b])


def mpileup_to_bins(model, mpileup_path_or_bytes, fasta_path, fai_text, out_dir, contigs=None, *, alt_info=True, matrix_dtype="int16", min_af=0.12,
                    indel_min_af=None, min_coverage=6, chunk_bytes=64 << 20, stats=None):
    """Stage s1 from the file the reference's stage 1 starts from: ONE mpileup text holding every contig (samtools mpileup BAM -o
    pileup_data, make_predict_data.sh:117) -> <out_dir>/<name>.pd.bin for every wanted contig the text holds, each byte for byte what
    contig_to_bin writes for the <name>.mpileup the splitter (DNA_ExtractChrPileupData) would have cut - make_predict_data.sh:167-234 in one
    call, the text read once.  Returns {name: sites} in text order.

    mpileup_path_or_bytes: a path, or bytes / mmap / uint8 array; contigs: the wanted names (None: every name of fai_text); model: only the
    holder of the context and the buffer sets (no weights needed).  The text is the ONE stream of call_mpileup (_stream_text_dev): the device
    finds the contig of every line and hands on key = (contig index << 36) | position; where call_mpileup runs the forward, this entry
    issues nsnp_pileup_window_records_keys and nsnp_pileup_alt_info_keys - reference bases and names out of the resident contig table, every
    site bounded by its OWN contig - into one of three pinned slots, and a writer thread cuts the slot's rows by contig (the key of every
    site comes back with them) and appends each piece to that contig's sitefile.PileupBinWriter.  The name in a position string is column
    0 of the emitting line (nsnp_mpileup_line_names_contigs), as in contig_to_bin.
    Which contigs get a file: a wanted contig the text holds, even one without a site (its file equals contig_to_bin of its lines); a wanted
    contig the text does not hold gets none, as the splitter writes none.  A wanted contig in two separate runs raises NanoSNPError, an
    empty line is refused, as in call_mpileup.
    The writers write to staging names inside out_dir, renamed into place only after the whole text has ended without error: on any error
    no staging or .tmp file of this call is left and whatever was in out_dir stays as it was.
    Restarts are of the WHOLE text: an alt_info text that outgrows its slot or a name table that is too small run it again with larger
    ones, and a count outside int16 runs it again as int32 - after which EVERY file of the run is int32 (make_pileup_bins over the split
    files would make only the overflowing contig's file int32).  stats: chunks, columns, sites, record_bytes, restarts; with
    stats["time_records"] = True also window_records_s / alt_info_s / record_chunks (HIP-event sums), as contig_to_bin reports them.
    Refused before anything is touched: a process group of more than one rank, NSNP_TOKENISE=host, no GPU (_bins_refusals); ValueError for
    a wanted name that is empty, holds NUL or is longer than 37 bytes."""
    return _mpileup_to_bins(model, mpileup_path_or_bytes, fasta_path, fai_text, out_dir, None, None, contigs=contigs, alt_info=alt_info,
                            matrix_dtype=matrix_dtype, min_af=min_af, indel_min_af=indel_min_af, min_coverage=min_coverage, chunk_bytes=chunk_bytes,
                            stats=stats)


def mpileup_to_bins_bed(model, mpileup_path_or_bytes, fasta_path, fai_text, out_dir, *, extended_bed=None, confident_bed=None, **kw):
    """mpileup_to_bins with the reference's two region filters over ALL contigs of the text (extended_bed / confident_bed: as call_mpileup_bed
    takes them): every <name>.pd.bin is byte for byte what make_pileup_bins(..., extended_bed=, confident_bed=) writes for the files the
    splitter would have cut, and the same set of files - a wanted contig the text holds gets one even when the extended BED drops all its
    lines (an empty file, as contig_to_bin writes for it).  Under an extended BED the name in a position string is still column 0 of the
    EMITTING line, the 16th kept line behind the centre: the name index of every line is compacted with the columns, which contig_to_bin
    does not do (it refuses such a text).  **kw and the refusals: as mpileup_to_bins; with both BEDs None this IS mpileup_to_bins."""
    return _mpileup_to_bins(model, mpileup_path_or_bytes, fasta_path, fai_text, out_dir, extended_bed, confident_bed, **kw)


def _mpileup_to_bins(model, mpileup_path_or_bytes, fasta_path, fai_text, out_dir, extended_bed, confident_bed, contigs=None, *, alt_info=True,
                     matrix_dtype="int16", min_af=0.12, indel_min_af=None, min_coverage=6, chunk_bytes=64 << 20, stats=None):
    """the one body of mpileup_to_bins and mpileup_to_bins_bed"""
    from concurrent.futures import ThreadPoolExecutor
    from . import _lib
    _bins_refusals()
    _check_matrix_dtype(matrix_dtype)
    names = [str(n) for n in (contigs if contigs is not None else fai_names(fai_text))]
    for n in names:
        _position_name(n)
    table = _lib.ContigTable(fasta=fasta_path, names=names, device=model.ctx.device)
    beds = None if extended_bed is None and confident_bed is None else _lib.BedTable(table, extended_bed, confident_bed, fai_text)
    st = _stream_stats(stats)
    with _text_of(mpileup_path_or_bytes) as src, ThreadPoolExecutor(max_workers=1) as pool:
        out = _staged_bins(out_dir, names, matrix_dtype, alt_info,
                           lambda staging, state: _records_pass(model, _KeyedRecords(model.ctx, table, beds, staging, alt_info), src, chunk_bytes,
                                                                min_af, indel_min_af, min_coverage, st, state, pool), st)
    st["sites"] = st.get("sites", 0) + sum(out.values())
    return out


# ---- one whole-genome mpileup text + a truth VCF -> every <chr>.td.bin (make_train_data.sh steps 4, 6 and 7) --------------------------------
class _TrainSlot(_RecSlot):
    """a _RecSlot with the labels of its rows (pinned), the label entry's counts (pinned) and the kept centres (device)"""
    def __init__(self, rows, blob_bytes, dev):
        import torch
        from ._lib import Context
        super().__init__(rows, blob_bytes)
        self.label = torch.empty((self.rows, Context.LABEL_WIDTH), dtype=torch.int32, pin_memory=True)
        self.lmeta = torch.zeros(4, dtype=torch.int64, pin_memory=True)
        self.kept = torch.empty(max(self.rows, 1), dtype=torch.int64, device=dev)


class _TrainStaging(_BinStaging):
    """_BinStaging for <name>.td.bin: sitefile.TrainBinWriter, and what only the rows themselves can say - that the sites of a contig are
    strictly ascending (NanoSNPError otherwise), and how many of the rows written are truth sites."""
    suffix = ".td.bin"

    def __init__(self, out_dir, names, matrix_dtype="int16", alt_info=True, truth_keys=None):
        super().__init__(out_dir, names, matrix_dtype, alt_info)
        self.truth_keys = np.zeros(0, np.int64) if truth_keys is None else truth_keys
        self.last, self.variants = {}, {}

    def _writer(self, cid):
        from . import sitefile
        return sitefile.TrainBinWriter(self.staging_path(cid), self.matrix_dtype, self.alt_info)

    def append(self, cid, x, position, label, blob=None, offsets=None, keys=None):
        from ._lib import KEY_SHIFT, NanoSNPError
        k = np.asarray(keys, np.int64)
        if k.size:
            back = np.flatnonzero(k[1:] <= k[:-1])
            at = int(k[0]) if (cid in self.last and k[0] <= self.last[cid]) else int(k[back[0] + 1]) if back.size else None
            if at is not None:
                raise NanoSNPError(f"{self.names[cid] if 0 <= cid < len(self.names) else cid}: the sites of a contig must be strictly ascending "
                                   f"(position {at & ((1 << KEY_SHIFT) - 1)} repeats or goes back)")
        if self.cur is None or self.cur_cid != cid:
            self._finish()
            if cid in self.done or not 0 <= cid < len(self.names):
                raise NanoSNPError(f"records: contig index {cid} outside the table or in two separate pieces")
            self.cur_cid, self.cur = cid, self._writer(cid)
        if self.alt_info:
            self.cur.append(x, position, label, blob, offsets)
        else:
            self.cur.append(x, position, label)
        if k.size:
            self.last[cid] = int(k[-1])
            at = np.searchsorted(self.truth_keys, k)
            hit = (at < self.truth_keys.size) & (self.truth_keys[np.minimum(at, max(self.truth_keys.size - 1, 0))] == k) if self.truth_keys.size else np.zeros(k.size, bool)
            self.variants[cid] = self.variants.get(cid, 0) + int(hit.sum())

    def abort(self):
        super().abort()
        self.last, self.variants = {}, {}


def _train_count_pass(model, ctx, text, table, chunk_bytes, min_af, indel_min_af, min_coverage, beds, truth, seed, state):
    """the count pass of mpileup_to_train_bins: the stream of the text with nothing but the count-mode label launch behind every chunk's
    selection -> int64 [n_contigs, 2] = {truth sites, other sites} per contig, or None when the pass has to be run again (state: name_cap)"""
    import torch
    from ._lib import NanoSNPError
    dev = torch.device("cuda", ctx.device)
    totals = torch.zeros((len(table), 2), dtype=torch.int64, device=dev)
    metas = []

    def records(k, counts, centers, cols, main):
        metas.append(ctx.pileup_label_sites_keys(cols.pos, centers, table, truth[0], truth[1], None, seed, counts=totals, stream=main,
                                                 want_label=False)[2])

    try:
        with host.gc_paused():
            _stream_text_dev(model, text, table, chunk_bytes, min_af, min_coverage, {}, None, indel_min_af=indel_min_af, records=records,
                             name_cap=state["name_cap"], beds=beds)
    except _NamesOverflow as e:
        state["name_cap"] = 2 * e.need + 64
        return None
    if metas and int(torch.stack(metas)[:, 3].max().item()):
        raise NanoSNPError("a selected site outside the columns or its contig, or at a reference byte other than A/C/G/T (label status)")
    return totals.cpu().numpy()


class _TrainLabels:
    """What _KeyedRecords does differently for mpileup_to_train_bins: truth = (device keys, device codes); thr: the device thresholds,
    or None - then every site is kept, N' == N is known on the host and the label launch simply goes in front of the record kernels on the
    compute stream.  With thresholds the label launch runs on a side stream (the chunk's selection is complete: its count has been
    read), the issuing thread waits for ITS event alone and reads N' from pinned memory, and the compute stream waits for that event -
    whatever else is queued on the compute stream (the record kernels of the chunk before) keeps running meanwhile."""

    def __init__(self, model, ctx, table, truth, thr, seed):
        import torch
        self.ctx, self.table, self.truth, self.thr, self.seed = ctx, table, truth, thr, seed
        self.dev = torch.device("cuda", ctx.device)
        self.side = None
        if thr is not None:
            self.side = getattr(model, "_label_stream", None)
            if self.side is None or self.side.device != self.dev:
                self.side = model._label_stream = torch.cuda.Stream(self.dev)

    def new_slot(self, rows, blob_bytes, main):
        slot = _TrainSlot(rows, blob_bytes, self.dev)
        if self.side is not None:
            # slot.kept comes out of the compute stream's pool: its block may be one a previous chunk's tensors (counts, depth, centres)
            # gave back while that chunk's record kernels are still queued on the compute stream and still read them.  The compute
            # stream's own later work is ordered behind those kernels; the side stream is not, and its first write into the new buffer
            # would be - so it waits once for everything queued on the compute stream so far (_text_chunk_sets does the same for the
            # copy stream).  Nothing in the steady state: a slot that is kept is not new.
            self.side.wait_stream(main)
        return slot

    def label(self, slot, centers, cols, main, st, flag):
        """the label launch of one chunk -> the centres the record kernels get (None: none)"""
        import time
        import torch
        ctx, truth = self.ctx, self.truth
        if self.thr is None:
            return ctx.pileup_label_sites_keys(cols.pos, centers, self.table, truth[0], truth[1], None, self.seed, out_center_idx=slot.kept,
                                               label=slot.label, meta=slot.lmeta, stream=main)[0]
        ctx.pileup_label_sites_keys(cols.pos, centers, self.table, truth[0], truth[1], self.thr, self.seed, out_center_idx=slot.kept,
                                    label=slot.label, meta=slot.lmeta, stream=self.side)
        labelled = torch.cuda.Event(); labelled.record(self.side)
        t_w = time.perf_counter()
        labelled.synchronize()
        st["wait_labels_s"] = st.get("wait_labels_s", 0.0) + time.perf_counter() - t_w
        main.wait_event(labelled)
        n_kept, _, _, status = slot.lmeta.tolist()
        if status:
            flag["status"] = 1
            return None
        st["dropped_sites"] = st.get("dropped_sites", 0) + int(centers.shape[0]) - n_kept
        return slot.kept[:n_kept] if n_kept else None


def mpileup_to_train_bins(model, mpileup_path_or_bytes, fasta_path, fai_text, truth_vcf, out_dir, contigs=None, *, extended_bed=None,
                          confident_bed=None, max_non_variant_ratio=5.0, seed=0, alt_info=True, matrix_dtype="int16", min_af=0.12,
                          indel_min_af=None, min_coverage=6, chunk_bytes=64 << 20, stats=None):
    """The training set of the PileupModel from the two files the reference's make_train_data.sh starts from: ONE mpileup text holding every
    contig and the truth VCF -> <out_dir>/<name>.td.bin for every wanted contig the text holds (sitefile.TrainBinWriter: position_matrix,
    position, label int32 [N,90], alt_info) - steps 4, 6 and 7 of that script (DNA_SplitVcf, DNA_CreateTrainData, make_bin_train_data.py)
    behind the steps mpileup_to_bins_bed already runs; with max_non_variant_ratio=None byte for byte sitefile.td_to_bin of the reference's
    <name>.td at -shuffle_tensors 0.

    truth_vcf: a path or the bytes of the VCF (truth.load_truth says how a row becomes a label, every quirk of the reference kept).  The
    text is the stream of mpileup_to_bins_bed; behind every chunk's selection nsnp_pileup_label_sites_keys looks every site up among the
    truth keys (resident on the device), labels it - a site no truth row names gets the homozygous-reference label of its base -, drops
    the surplus of such sites and hands the record kernels the centres that are left.
    max_non_variant_ratio (the reference's -maxinum_non_variant_ratio): None keeps every site in ONE pass.  A number runs a count pass over
    the text first (the same stream, only the counting launch behind each selection); per contig max_nv = int(variants * ratio), and a
    contig with more non-variant sites than that keeps such a site when (hash(key, seed) >> 11) < (max_nv << 53) // non_variants - a
    contig with sites but without a truth site keeps nothing, as the reference's arithmetic gives.
    Where this departs from the reference: rows stay in text order (no shuffle); the subsample is a seeded function of
    the key, the same set for every chunk layout and run; the sites of a contig must be strictly ascending (NanoSNPError); the
    confident_* recall line of the reference's log is not computed.
    Everything else - contigs, the BEDs, alt_info, matrix_dtype, the staging names renamed only on success, restarts of the whole text, the
    set of files, the refusals (_bins_refusals) - as mpileup_to_bins_bed.  stats: as there, plus count_pass_s, wait_labels_s, dropped_sites.
    Returns {name: dict(sites=, variants=, non_variants=, kept=, ratio=, truth=, recall=)} in text order: the numbers of the reference's two
    log lines (candidate sites that are / are not truth variants, the subsample ratio, the contig's truth variants and the share of them
    among the sites) and the rows written."""
    import time
    import torch
    from concurrent.futures import ThreadPoolExecutor
    from . import _lib
    from . import truth as _truth
    _bins_refusals()
    _check_matrix_dtype(matrix_dtype)
    if max_non_variant_ratio is not None and not float(max_non_variant_ratio) >= 0.0:
        raise ValueError("max_non_variant_ratio: None or a number >= 0")
    names = [str(n) for n in (contigs if contigs is not None else fai_names(fai_text))]
    for n in names:
        _position_name(n)
    ctx = model.ctx
    dev = torch.device("cuda", ctx.device)
    table = _lib.ContigTable(fasta=fasta_path, names=names, device=ctx.device)
    t_keys, t_codes, t_counts = _truth.load_truth(truth_vcf, table)
    truth = (torch.from_numpy(t_keys).to(dev), torch.from_numpy(t_codes.view(np.int32)).to(dev))
    beds = None if extended_bed is None and confident_bed is None else _lib.BedTable(table, extended_bed, confident_bed, fai_text)
    st = _stream_stats(stats)
    with _text_of(mpileup_path_or_bytes) as src:
        counted = thr = ratios = None
        if max_non_variant_ratio is not None:
            t0 = time.perf_counter()
            cstate = dict(name_cap=1024)
            while counted is None:
                counted = _train_count_pass(model, ctx, src, table, chunk_bytes, min_af, indel_min_af, min_coverage, beds, truth, seed, cstate)
            st["count_pass_s"] = st.get("count_pass_s", 0.0) + time.perf_counter() - t0
            thr_list, ratios = _truth.keep_thresholds(counted[:, 0], counted[:, 1], max_non_variant_ratio)
            thr = torch.tensor(thr_list, dtype=torch.int64, device=dev) if thr_list else None
        labels = _TrainLabels(model, ctx, table, truth, thr, seed)
        made = []

        def staging_of(*a):
            made.append(_TrainStaging(*a, truth_keys=t_keys))
            return made[-1]

        with ThreadPoolExecutor(max_workers=1) as pool:
            out = _staged_bins(out_dir, names, matrix_dtype, alt_info,
                               lambda staging, state: _records_pass(model, _KeyedRecords(ctx, table, beds, staging, alt_info, train=labels), src,
                                                                    chunk_bytes, min_af, indel_min_af, min_coverage, st, state, pool),
                               st, staging_cls=staging_of)
        st["sites"] = st.get("sites", 0) + sum(out.values())
        result = {}
        for name, kept in out.items():
            cid = names.index(name)
            variants = made[-1].variants.get(cid, 0)
            if counted is None:
                sites, non_variants, ratio = kept, kept - variants, 1.0
            else:
                if int(counted[cid, 0]) != variants:
                    raise _lib.NanoSNPError(f"{name}: the count pass saw {int(counted[cid, 0])} truth sites, the write pass wrote {variants}")
                sites, non_variants, ratio = int(counted[cid].sum()), int(counted[cid, 1]), ratios[cid]
            n_truth = int(t_counts[cid])
            result[name] = dict(sites=sites, variants=variants, non_variants=non_variants, kept=kept, ratio=ratio, truth=n_truth,
                                recall=variants / n_truth if n_truth else float("nan"))
        return result
