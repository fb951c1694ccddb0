"""Input pipeline on the engine's host parser: text files -> device batches.

Mirrors the reference's RecDataset readers (same constructor shape: file_list, config) for
  models/rank/deepfm/criteo_reader.py:21-103 / dcn_v2/reader.py  (slot text)   -> SlotTextReader
  models/rank/dnn/benchmark_reader.py:35-54                       (raw Criteo)  -> CriteoTsvReader
but parses whole files in C++ (librecengine.so, multi-threaded) into pinned host buffers and ships each
batch with one async copy, instead of a Python loop per line + a 28-array collate per sample.
Batches have the layout the kernels take: label [B,1] i64, ids [B,26] i64 (= concat(sparse_inputs,1)),
dense [B,13] f32.  drop_last=True as tools/utils/utils_single.py:104-110 builds the DataLoader.
"""
import ctypes as C
import mmap
import os
import queue
import threading
import time

import numpy as np
import torch

from ._lib import check, lib

CONT_MIN = [0, -3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]                      # benchmark_reader.py:23
CONT_DIFF = [20, 603, 100, 50, 64000, 500, 100, 50, 500, 10, 10, 10, 50]  # benchmark_reader.py:25
HASH_DIM = 1000001                                                        # benchmark_reader.py:26


def _alloc(n, S, Dn, pinned):
    pin = pinned and torch.cuda.is_available()
    label = torch.empty(n, dtype=torch.int64, pin_memory=pin)
    ids = torch.empty(n, S, dtype=torch.int64, pin_memory=pin)
    dense = torch.empty(n, max(Dn, 1), dtype=torch.float32, pin_memory=pin)
    return label, ids, dense


def _close_mmap(mm):
    """Closes a text mapping.  If the parser raised, the traceback's frames may still hold the NumPy view _buf()
    exported from it and mmap.close() raises BufferError('cannot close exported pointers exist') — which would mask
    the parse error that matters.  Then the mapping is left to the garbage collector."""
    try:
        mm.close()
    except BufferError:
        pass


def _buf(data):
    """(char pointer, length, keep-alive) of the text: a bytes object, or any buffer — the readers hand in an mmap of
    the file, so the parser threads read the page cache directly and no copy of the text is made."""
    if isinstance(data, bytes):
        return data, len(data), data
    arr = np.frombuffer(data, np.uint8)
    return C.c_char_p(arr.ctypes.data), arr.size, arr


def _count_lines(data, threads):
    n = C.c_int64(0)
    ptr, ln, _keep = _buf(data)
    check(lib().rec_count_lines(ptr, ln, threads, C.byref(n)), "rec_count_lines")
    return max(int(n.value), 1)


def blank_lines(data, threads=0):
    """Indices of the whitespace-only lines of the text (sorted numpy int64 array; usually empty)."""
    ptr, ln, _keep = _buf(data)
    n = C.c_int64(0)
    check(lib().rec_blank_lines(ptr, ln, threads, 0, None, C.byref(n)), "rec_blank_lines")
    out = np.empty(max(int(n.value), 1), np.int64)
    if n.value:
        check(lib().rec_blank_lines(ptr, ln, threads, int(n.value), out.ctypes.data_as(C.c_void_p), C.byref(n)),
              "rec_blank_lines")
    return out[: int(n.value)]


def csr_cut(pieces, num_slots, threads=0):
    """One batch from consecutive line ranges of parse_feasign_slots results: pieces = [(values, lod, base, l0, l1)].
    -> (values, lod [num_slots, lines + 1], base [num_slots + 1]) host tensors (rec_csr_cut)."""
    P = len(pieces)
    nl = sum(l1 - l0 for _, _, _, l0, l1 in pieces)
    total = sum(int((lod[:, l1] - lod[:, l0]).sum()) for _, lod, _, l0, l1 in pieces)
    out_v = torch.empty(max(total, 1), dtype=torch.int64)
    out_l = torch.empty(num_slots, nl + 1, dtype=torch.int64)
    out_b = torch.empty(num_slots + 1, dtype=torch.int64)
    arr = lambda xs: (C.c_void_p * P)(*xs)
    i64 = lambda xs: (C.c_int64 * P)(*xs)
    check(lib().rec_csr_cut(num_slots, P, arr([v.data_ptr() for v, _, _, _, _ in pieces]),
                            arr([l.data_ptr() for _, l, _, _, _ in pieces]), i64([l.stride(0) for _, l, _, _, _ in pieces]),
                            arr([b.data_ptr() for _, _, b, _, _ in pieces]), i64([p[3] for p in pieces]),
                            i64([p[4] for p in pieces]), threads, C.c_void_p(out_v.data_ptr()), out_v.numel(),
                            C.c_void_p(out_l.data_ptr()), C.c_void_p(out_b.data_ptr())), "rec_csr_cut")
    return out_v[:total], out_l, out_b


def parse_slot_text(data: bytes, n_sparse=26, n_dense=13, log1p_dense=False, threads=0, pinned=False):
    """-> (label [n] i64, ids [n,S] i64, dense [n,Dn] f32) host tensors."""
    cap = _count_lines(data, threads)
    label, ids, dense = _alloc(cap, n_sparse, n_dense, pinned)
    n = C.c_int64(0)
    ptr, ln, _keep = _buf(data)
    check(lib().rec_parse_slot_text(ptr, ln, n_sparse, n_dense, int(log1p_dense), cap, threads,
                                    C.c_void_p(label.data_ptr()), C.c_void_p(ids.data_ptr()),
                                    C.c_void_p(dense.data_ptr()), C.byref(n)), "rec_parse_slot_text")
    return label[: n.value], ids[: n.value], dense[: n.value, :n_dense]


def parse_criteo_tsv(data: bytes, n_dense=13, n_sparse=26, hash_dim=HASH_DIM, threads=0, pinned=False):
    cap = _count_lines(data, threads)
    label, ids, dense = _alloc(cap, n_sparse, n_dense, pinned)
    cmin = np.asarray(CONT_MIN[:n_dense], np.float32)
    cdiff = np.asarray(CONT_DIFF[:n_dense], np.float32)
    n = C.c_int64(0)
    ptr, ln, _keep = _buf(data)
    check(lib().rec_parse_criteo_tsv(ptr, ln, n_dense, n_sparse, cmin.ctypes.data_as(C.c_void_p),
                                     cdiff.ctypes.data_as(C.c_void_p), hash_dim, cap, threads,
                                     C.c_void_p(label.data_ptr()), C.c_void_p(ids.data_ptr()),
                                     C.c_void_p(dense.data_ptr()), C.byref(n)), "rec_parse_criteo_tsv")
    return label[: n.value], ids[: n.value], dense[: n.value, :n_dense]


def parse_feasign_slots(data: bytes, first_slot=1, num_slots=301, hash_rows=0, threads=0):
    """Multi-value slot lines (slot_dnn/queuedataset_reader.py:56-82) -> slot-major CSR, host tensors:
    (values [total] i64, lod [num_slots, n+1] i64, slot_base [num_slots+1] i64, n lines) — slot s of line b is
    values[slot_base[s] + lod[s,b] : slot_base[s] + lod[s,b+1]]; with hash_rows > 0 the values are table rows."""
    cap = _count_lines(data, threads)
    ptr, ln, _keep = _buf(data)
    nc = C.c_int64(0)
    check(lib().rec_count_byte(ptr, ln, ord(":"), threads, C.byref(nc)), "rec_count_byte")
    bound = int(nc.value) + cap * num_slots             # every token + one padding id per (line, slot)
    values = torch.empty(max(bound, 1), dtype=torch.int64)
    lod = torch.empty(num_slots, cap + 1, dtype=torch.int64)       # the parser writes every offset of the n lines
    base = torch.zeros(num_slots + 1, dtype=torch.int64)
    n, nv = C.c_int64(0), C.c_int64(0)
    check(lib().rec_parse_feasign_slots(ptr, ln, int(first_slot), int(num_slots), int(hash_rows), cap,
                                        values.numel(), threads, C.c_void_p(values.data_ptr()),
                                        C.c_void_p(lod.data_ptr()), C.c_void_p(base.data_ptr()), C.byref(n),
                                        C.byref(nv)), "rec_parse_feasign_slots")
    return values[: nv.value], lod[:, : n.value + 1], base, int(n.value)


class FeasignSlotReader:
    """slot_dnn/queuedataset_reader.py Reader over a file list: yields, per batch of `batch_size` lines (drop_last),
    (values, lod [num_slots, B+1], slot_base [num_slots+1]) on `device` — slot s of the batch feeds one
    rec_emb_gather_sumpool launch: ids = values[slot_base[s]:slot_base[s+1]], lod = lod[s]."""

    def __init__(self, file_list, batch_size, device="cuda", first_slot=1, num_slots=301, hash_rows=0, threads=0):
        self.file_list, self.batch_size, self.device = list(file_list), batch_size, device
        self.kw = dict(first_slot=first_slot, num_slots=num_slots, hash_rows=hash_rows, threads=threads)

    def __iter__(self):
        for values, lod, base in feasign_batches(self.file_list, self.batch_size, **self.kw):
            yield tuple(t.to(self.device, non_blocking=True) for t in (values, lod, base))


def feasign_batches(file_list, batch_size, first_slot=1, num_slots=301, hash_rows=0, threads=0):
    """Host batches (values, lod [num_slots, B+1], slot_base) of `batch_size` lines over a file list in the multi-value
    `feasign:slot` format: every file is parsed ONCE, whole (mmap'ed text, all threads), and the batches are cut from
    the parse by rec_csr_cut — lines are never split or re-joined in python.  Batching as the reference's datasets do
    it: lines accumulate across files, whitespace-only lines are skipped, the last partial batch is dropped."""
    B = batch_size
    pieces, have = [], 0              # (values, lod, base, first line, end line) ranges not yet batched
    for path in file_list:
        if os.path.getsize(path) == 0:
            continue
        with open(path, "rb") as f:
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            try:
                values, lod, base, n = parse_feasign_slots(mm, first_slot, num_slots, hash_rows, threads)
                blank = blank_lines(mm, threads).tolist()
            finally:
                _close_mmap(mm)
        edges = [-1] + [b for b in blank if b < n] + [n]       # runs of real lines between the (rare) blank ones
        for a, z in zip(edges[:-1], edges[1:]):
            lo = a + 1
            while have + (z - lo) >= B:
                take = B - have
                pieces.append((values, lod, base, lo, lo + take))
                yield csr_cut(pieces, num_slots, threads)
                pieces, have, lo = [], 0, lo + take
            if lo < z:
                pieces.append((values, lod, base, lo, z))
                have += z - lo


class _FileBatches:
    last_trace = None

    def __init__(self, file_list, batch_size, device, parse, shard=None):
        self.file_list = list(file_list)
        if shard is not None:                      # criteo_reader.py:30-43: files split by worker
            rank, world = shard
            if len(self.file_list) < world:
                raise ValueError("The number of data files is less than the number of workers")
            blk = len(self.file_list) // world
            mine = self.file_list[rank * blk:(rank + 1) * blk]
            if rank < len(self.file_list) - blk * world:
                mine.append(self.file_list[-(rank + 1)])
            self.file_list = mine
        self.batch_size, self.device, self.parse = batch_size, device, parse

    def _load(self, path):
        """One file -> host tensors.  The text is mmap'ed, not read(): the parser's threads walk the page cache
        directly (a read() of the file alone was 51 ms per 277 MB, four times the 12 ms the parse takes)."""
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            if size == 0:
                return self.parse(b"")
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            try:
                return self.parse(mm)
            finally:
                _close_mmap(mm)

    def _files(self):
        """Parsed files in order; the NEXT files are read and parsed by background threads (the parser is a C call that
        releases the GIL) while the caller trains on the current one — started NOW, not at the first next(): iter(reader)
        begins the pass.  REC_READER_PRODUCERS (default 1) producers take the files round-robin (measured: the parser
        already uses every core, two producers only slow each other — profiles/r04_trainer_level.txt) and the consumer
        takes their results in file order."""
        nprod = max(1, min(int(os.environ.get("REC_READER_PRODUCERS", "1")), len(self.file_list) or 1))
        queues = [queue.Queue(maxsize=1) for _ in range(nprod)]
        stop = threading.Event()
        # REC_READER_TRACE=1: (file, load seconds, seconds blocked on the queue) of the newest pass over the files
        trace = _FileBatches.last_trace = [] if os.environ.get("REC_READER_TRACE") else None

        def put(q, item):
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    pass
            return False

        def produce(k):
            q = queues[k]
            try:
                for path in self.file_list[k::nprod]:
                    t0 = time.perf_counter()
                    item = self._load(path)
                    t1 = time.perf_counter()
                    if not put(q, item):
                        return
                    if trace is not None:
                        trace.append([os.path.basename(path), t1 - t0, time.perf_counter() - t1])
                item = None
            except BaseException as e:           # surfaces in the consumer
                item = e
            put(q, item)

        for k in range(nprod):
            threading.Thread(target=produce, args=(k,), daemon=True).start()
        return _StoppingIter(self._consume(queues, nprod, stop), stop)

    def _consume(self, queues, nprod, stop):
        try:
            for i in range(len(self.file_list)):
                item = queues[i % nprod].get()
                if isinstance(item, BaseException):
                    raise item
                if item is None:                 # a producer ran out early: cannot happen with a fixed file list
                    return
                yield item
            for q in queues:                     # every producer ends with None or an exception
                item = q.get()
                if isinstance(item, BaseException):
                    raise item
        finally:
            stop.set()

    def __iter__(self):
        """iter(reader) starts reading and parsing the first files right away; the batches come from the returned
        generator.  (The trainer creates the NEXT epoch's iterator before it drains the device and writes the checkpoint
        of this one, so an epoch does not begin with an idle device waiting for its first file.)"""
        return self._batches(self._files())

    def _batches(self, files):
        B = self.batch_size
        carry = None
        for label, ids, dense in files:
            if carry is not None:
                label, ids, dense = (torch.cat([c, x]) for c, x in zip(carry, (label, ids, dense)))
            n = label.shape[0]
            for lo in range(0, n - B + 1, B):
                yield tuple(t[lo:lo + B].to(self.device, non_blocking=True) for t in
                            (label.view(-1, 1), ids, dense))
            rem = n % B
            carry = (label[n - rem:], ids[n - rem:], dense[n - rem:]) if rem else None


class _StoppingIter:
    """The file iterator of _FileBatches: its producers are started eagerly, so the stop flag must follow the lifetime of
    THIS object — an iterator that is dropped before (or between) next() calls stops them, where a bare generator's
    `finally` only runs once the generator has been started."""

    def __init__(self, gen, stop):
        self._gen, self._stop = gen, stop

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        self._stop.set()
        self._gen.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SlotTextReader(_FileBatches):
    """criteo_reader.py RecDataset: yields (label [B,1], ids [B,26], dense [B,13]) on `device`."""

    def __init__(self, file_list, batch_size, device="cuda", log1p_dense=False, shard=None, threads=0):
        super().__init__(file_list, batch_size, device,
                         lambda data: parse_slot_text(data, 26, 13, log1p_dense, threads, pinned=True), shard)


class CriteoTsvReader(_FileBatches):
    """benchmark_reader.py Reader: raw Criteo TSV, min-max dense scaling, xxh32 feature hashing."""

    def __init__(self, file_list, batch_size, device="cuda", hash_dim=HASH_DIM, shard=None, threads=0):
        super().__init__(file_list, batch_size, device,
                         lambda data: parse_criteo_tsv(data, 13, 26, hash_dim, threads, pinned=True), shard)


def parse_avazu_csv(data, n_fields=24):
    """flen/avazu_reader.py:30-49: comma-separated integer lines; a line with any other field count is skipped silently.
    -> (label [n] i64 = the LAST column, ids [n, n_fields - 1] i64 = the columns in front of it, an empty [n, 0] dense)."""
    import numpy as np
    rows = [r for r in (line.strip().split(",") for line in bytes(data).decode().splitlines()) if len(r) == n_fields]
    arr = np.asarray(rows, dtype=str).astype(np.int64) if rows else np.zeros((0, n_fields), np.int64)
    t = torch.from_numpy(arr)
    return t[:, -1].contiguous(), t[:, :-1].contiguous(), torch.zeros(t.shape[0], 0)


class AvazuReader(_FileBatches):
    """flen/avazu_reader.py RecDataset with the batching of the other readers (drop_last, rank sharding of the files):
    yields (label [B,1], ids [B,23]) on `device`.  Column 0 of ids is in the batch; the net ignores it."""

    def __init__(self, file_list, batch_size, device="cuda", shard=None):
        super().__init__(file_list, batch_size, device, parse_avazu_csv, shard)

    def _batches(self, files):
        for label, ids, _ in super()._batches(files):
            yield label, ids


class AutofisReader:
    """autofis/criteo_reader.py RecDataset: the data directory holds two whitespace-separated text files, `*x.txt` with
    S int64 ids per line and `*y.txt` with one label per line.  Yields (label [B,1], ids [B,S]) on `device` with the
    batching of the other readers (drop_last); len() is the number of batches (the trainer's lr decay needs it).  shard =
    (rank, world): every rank takes its contiguous block of the samples."""

    def __init__(self, file_list, batch_size, device="cuda", shard=None):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        x = y = None
        for path in self.file_list:                                      # criteo_reader.py:24-28
            if path.endswith("x.txt"):
                x = np.loadtxt(path, dtype=np.int64, ndmin=2)
            elif path.endswith("y.txt"):
                y = np.loadtxt(path, dtype=np.int64, ndmin=1)
        if x is None or y is None:
            raise ValueError("autofis needs a *x.txt and a *y.txt file, got %s" % [os.path.basename(f) for f in file_list])
        if len(x) != len(y):
            raise ValueError("%d lines of ids against %d labels" % (len(x), len(y)))
        if shard is not None:
            rank, world = shard
            blk = len(x) // world
            x, y = x[rank * blk:(rank + 1) * blk], y[rank * blk:(rank + 1) * blk]
        self.x, self.y = torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(np.ascontiguousarray(y)).reshape(-1, 1)

    def __len__(self):
        return len(self.x) // self.batch_size

    def __iter__(self):
        B = self.batch_size
        for i in range(len(self)):
            yield self.y[i * B:(i + 1) * B].to(self.device), self.x[i * B:(i + 1) * B].to(self.device)


class DinReader:
    """models/rank/din/dinReader.py RecDataset: lines "hist items;hist cats;target item;target cat;label".
    Groups of 20*batch_size samples are sorted by history length (stable) and cut into batches padded to the
    batch's longest history; yields (hist_item [B,T], hist_cat [B,T], target_item [B], target_cat [B],
    label [B,1] f32, mask [B,T,1] i64 (0 / -1e9), target_item_seq [B,T], target_cat_seq [B,T]) on `device` —
    the eight feeds of din/dygraph_model.py:47-56.  (The reference also scans the files for the longest
    history and writes it to ./tmp.txt, dinReader.py:29-43 — an unused side effect that is not reproduced.)"""

    def __init__(self, file_list, batch_size, device="cuda"):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device

    def _emit(self, group, upto):
        B = self.batch_size
        lens = np.fromiter((len(g[0]) for g in group), dtype=np.int64, count=len(group))
        order = np.argsort(lens, kind="stable")
        for i in range(0, upto, B):
            idx = order[i:i + B]
            T = int(lens[idx].max())
            item = np.zeros((len(idx), T), np.int64)
            cat = np.zeros((len(idx), T), np.int64)
            for r, k in enumerate(idx):
                item[r, :lens[k]] = group[k][0]
                cat[r, :lens[k]] = group[k][1]
            ti = np.array([group[k][2] for k in idx], np.int64)
            tc = np.array([group[k][3] for k in idx], np.int64)
            label = np.array([group[k][4] for k in idx], np.float32).reshape(-1, 1)
            mask = np.where(np.arange(T)[None, :] < lens[idx][:, None], 0, -1000000000).astype(np.int64)
            arrs = (item, cat, ti, tc, label, mask.reshape(-1, T, 1), np.repeat(ti[:, None], T, 1),
                    np.repeat(tc[:, None], T, 1))
            yield tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True) for a in arrs)

    def __iter__(self):
        group, gsz = [], self.batch_size * 20
        for path in self.file_list:
            with open(path, "r") as f:
                for line in f:
                    parts = line.strip().split(";")
                    if len(parts) < 5:
                        continue
                    group.append((np.array(parts[0].split(), np.int64), np.array(parts[1].split(), np.int64),
                                  int(parts[2]), int(parts[3]), float(parts[4])))
                    if len(group) == gsz:
                        yield from self._emit(group, gsz)
                        group = []
        if group:
            yield from self._emit(group, len(group) - len(group) % self.batch_size)


class DienReader:
    """models/rank/dien/dien_reader.py RecDataset: DIN's text format plus negative sampling.  Lines whose largest item id
    exceeds item_count (or category id cat_count) are dropped; the kept samples are shuffled with random.seed(12345);
    groups of 20*batch_size are sorted by history length (stable) and cut into batches padded to the batch's longest
    history, and a batch whose longest history is below 2 is skipped.  Negatives come from two candidate pools (10000
    items, 1000 categories) that persist over the reader's life and are drawn with Python's `random` in the reference's
    call order — including its slip of writing a sample's CATEGORIES into the ITEM pool once the category pool is full
    (dien_reader.py:137), and its slice assignment of len+1 slots, which shortens the pool by one.  Yields the ten feeds of
    dien/dygraph_model.py:46-57 on `device`: hist_item, hist_cat [B,T] i64, target_item, target_cat [B] i64, label [B]
    f32, mask [B,T,1] f32 (0 / -1e9), target_item_seq, target_cat_seq, neg_item, neg_cat [B,T] i64.  (The reference also
    writes the longest history to ./tmp.txt — an unused side effect that is not reproduced.)"""
    MAX_NEG_ITEM, MAX_NEG_CAT = 10000, 1000

    def __init__(self, file_list, batch_size, device="cuda", item_count=63001, cat_count=801):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        self.item_count, self.cat_count = item_count, cat_count
        self.pool_item, self.pool_cat = [], []

    def _negatives(self, sample, T):
        import random
        hist, cats = sample[0], sample[1]
        if len(self.pool_item) < self.MAX_NEG_ITEM:
            self.pool_item.extend(hist)
            del self.pool_item[self.MAX_NEG_ITEM:]
        else:
            at = random.randint(0, self.MAX_NEG_ITEM - len(hist) - 1)
            self.pool_item[at:at + len(hist) + 1] = hist
        if len(self.pool_cat) < self.MAX_NEG_CAT:
            self.pool_cat.extend(cats)
            del self.pool_cat[self.MAX_NEG_CAT:]
        else:
            at = random.randint(0, self.MAX_NEG_CAT - len(cats) - 1)
            self.pool_item[at:at + len(cats) + 1] = cats              # the reference's slip: the ITEM pool
        ni = [self.pool_item[random.randint(0, len(self.pool_item) - 1)] for _ in range(T)]
        nc = [self.pool_cat[random.randint(0, len(self.pool_cat) - 1)] for _ in range(T)]
        return ni, nc

    def _emit(self, group, upto):
        B = self.batch_size
        order = sorted(range(len(group)), key=lambda i: len(group[i][0]))       # stable, as sorted() in the reference
        for i in range(0, upto, B):
            b = [group[k] for k in order[i:i + B]]
            T = max(len(x[0]) for x in b)
            if T < 2:
                continue
            item, cat = np.zeros((len(b), T), np.int64), np.zeros((len(b), T), np.int64)
            ni, nc = np.zeros((len(b), T), np.int64), np.zeros((len(b), T), np.int64)
            lens = np.array([len(x[0]) for x in b])
            for r, x in enumerate(b):
                item[r, :len(x[0])], cat[r, :len(x[1])] = x[0], x[1]
                ni[r], nc[r] = self._negatives(x, T)
            ti, tc = np.array([x[2] for x in b], np.int64), np.array([x[3] for x in b], np.int64)
            label = np.array([x[4] for x in b], np.float32)
            mask = np.where(np.arange(T)[None, :] < lens[:, None], 0.0, -1e9).astype(np.float32).reshape(-1, T, 1)
            arrs = (item, cat, ti, tc, label, mask, np.repeat(ti[:, None], T, 1), np.repeat(tc[:, None], T, 1), ni, nc)
            yield tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device, non_blocking=True) for a in arrs)

    def __iter__(self):
        import random
        data = []
        for path in self.file_list:
            with open(path, "r") as f:
                for line in f:
                    parts = line.strip().split(";")
                    if len(parts) != 5:
                        continue
                    hist, cats = [int(x) for x in parts[0].split()], [int(x) for x in parts[1].split()]
                    if max(hist) > self.item_count or max(cats) > self.cat_count:
                        continue
                    data.append((hist, cats, int(parts[2]), int(parts[3]), float(parts[4])))
        random.seed(12345)
        random.shuffle(data)
        gsz = self.batch_size * 20
        full = len(data) - len(data) % gsz
        for s in range(0, full, gsz):
            yield from self._emit(data[s:s + gsz], gsz)
        tail = data[full:]
        if tail:
            yield from self._emit(tail, len(tail) - len(tail) % self.batch_size)


class AlimamaReader:
    """models/rank/dmr/alimama_reader.py RecDataset with the batching of the other readers (drop_last over the
    concatenation of the files): comma-separated lines of 267 fields; '' and NULL (any case) read as 0; every value goes
    through float32 and is then truncated to int64, as np.array(l).astype('float32') followed by
    dygraph_model.py:63's astype('int64') does.  Yields (sparse [B, 267] i64, price [B, 1] f32 = column 264) on
    `device`; the label is the last column of sparse.  A line with another field count is an error (the reference's
    batching would fail on it)."""
    FIELDS, PRICE_COL = 267, 264

    def __init__(self, file_list, batch_size, device="cuda"):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device

    def _rows(self):
        for path in self.file_list:
            with open(path, "r") as f:
                for no, line in enumerate(f, 1):
                    parts = line.strip().split(",")
                    if parts == [""]:
                        continue
                    if len(parts) != self.FIELDS:
                        raise ValueError("%s:%d has %d fields, expected %d" % (path, no, len(parts), self.FIELDS))
                    yield ["0" if x == "" or x.upper() == "NULL" else x for x in parts]

    def __iter__(self):
        group = []
        for row in self._rows():
            group.append(row)
            if len(group) == self.batch_size:
                arr = np.asarray(group).astype(np.float32)
                group = []
                sparse = torch.from_numpy(arr.astype(np.int64))
                price = torch.from_numpy(np.ascontiguousarray(arr[:, self.PRICE_COL:self.PRICE_COL + 1]))
                yield sparse.to(self.device, non_blocking=True), price.to(self.device, non_blocking=True)


class AmazonBSTReader:
    """models/rank/bst/amazon_reader.py RecDataset with the batching of the other readers (drop_last over the
    concatenation of the files): lines of `slot:id` tokens for the slots label, userid, history, cate, position, target,
    target_cate, target_position; tokens of other slots are skipped; a slot missing from a line reads as [0].  history,
    cate and position are padded with 0 to the longest history found in ALL files of the list (the reference pre-scans the
    whole list before it yields), so the sequence length is a property of the data set, not of the batch.  Yields the
    eight int64 arrays of bst/dygraph_model.py:63-73 on `device`: label, userid [B,1], history, cate, position [B,T],
    target, target_cate, target_position [B,1]."""
    SLOTS = ("label", "userid", "history", "cate", "position", "target", "target_cate", "target_position")
    PADDED = (2, 3, 4)

    def __init__(self, file_list, batch_size, device="cuda"):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device

    def max_len(self):
        """The longest history of the file list (amazon_reader.py:46-56)."""
        longest = 0
        for path in self.file_list:
            with open(path, "r") as f:
                for line in f:
                    longest = max(longest, sum(1 for tok in line.strip().split(" ") if tok.split(":")[0] == "history"))
        return longest

    def _rows(self, max_len):
        index = {s: i for i, s in enumerate(self.SLOTS)}
        for path in self.file_list:
            with open(path, "r") as f:
                for line in f:
                    out = [[] for _ in self.SLOTS]
                    for tok in line.strip().split(" "):
                        parts = tok.split(":")
                        if parts[0] in index:
                            out[index[parts[0]]].append(int(parts[1]))
                    out = [v or [0] for v in out]
                    yield [np.asarray(v + [0] * (max_len - len(v)) if i in self.PADDED else v, np.int64)
                           for i, v in enumerate(out)]

    def __iter__(self):
        group = []
        for row in self._rows(self.max_len()):
            group.append(row)
            if len(group) == self.batch_size:
                arrs = [np.stack([r[i] for r in group]) for i in range(len(self.SLOTS))]
                group = []
                yield tuple(torch.from_numpy(a).to(self.device, non_blocking=True) for a in arrs)


class CensusReader:
    """models/multitask/{mmoe,ple}/census_reader.py RecDataset with the batching of the other readers (drop_last over the
    concatenation of the files): comma-separated lines of 2 + feature_size numbers — label_marital, label_income, then the
    features, each float32(float(token)).  Yields (features [B, F] f32, label_income [B, 1] f32, label_marital [B, 1] f32)
    on `device`, the order of dygraph_model.py's create_feeds.  A label other than 0 or 1 is a ValueError naming file and
    line: the reference yields an empty label array there and fails later, in the collate (and truncates a fractional
    label with int(), 0.5 -> 0: also refused here).  The feature
    count is the first line's; a line with another count is an error."""

    def __init__(self, file_list, batch_size, device="cuda"):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device

    def _rows(self):
        width = None
        for path in self.file_list:
            with open(path, "r") as f:
                for no, line in enumerate(f, 1):
                    parts = line.strip().split(",")
                    if parts == [""]:
                        continue
                    vals = list(map(float, parts))
                    if len(vals) < 3 or (width is not None and len(vals) != width):
                        raise ValueError("%s:%d has %d fields, expected %s" % (path, no, len(vals), width or "at least 3"))
                    width = len(vals)
                    for what, v in (("label_marital", vals[0]), ("label_income", vals[1])):
                        if v not in (0.0, 1.0):
                            raise ValueError("%s:%d: %s is %r, expected 0 or 1" % (path, no, what, v))
                    yield np.array(vals[2:]).astype(np.float32), vals[1], vals[0]

    def __iter__(self):
        group = []
        for row in self._rows():
            group.append(row)
            if len(group) == self.batch_size:
                feats = torch.from_numpy(np.stack([r[0] for r in group]))
                income = torch.tensor([[r[1]] for r in group], dtype=torch.float32)
                marital = torch.tensor([[r[2]] for r in group], dtype=torch.float32)
                group = []
                yield tuple(t.to(self.device, non_blocking=True) for t in (feats, income, marital))


class AliCCPReader:
    """models/multitask/esmm/esmm_reader.py and escm2/escm_reader.py RecDataset (the two files are identical) with the
    batching of the other readers (drop_last over the concatenation of the files).  A line is `_, ctr, ctcvr, _,
    field:feat, ...`; the features of the 23 fields below are kept in line order, every other field is dropped, and each
    field is cut to max_len ids (hyper_parameters.max_len, default 3) or padded with 0.  Yields (ids [B, 23, max_len] i64,
    click [B] i64, buy [B] i64) on `device`: ids[:, f, :] is the reference's f-th per-field array."""
    FIELDS = ("101", "109_14", "110_14", "127_14", "150_14", "121", "122", "124", "125", "126", "127", "128", "129", "205",
              "206", "207", "210", "216", "508", "509", "702", "853", "301")

    def __init__(self, file_list, batch_size, device="cuda", max_len=3):
        self.file_list, self.batch_size, self.device, self.max_len = list(file_list), int(batch_size), device, int(max_len)
        self.index = {f: i for i, f in enumerate(self.FIELDS)}

    def _rows(self):
        L = self.max_len
        for path in self.file_list:
            with open(path, "r") as f:
                for no, line in enumerate(f, 1):
                    parts = line.strip().split(",")
                    if parts == [""]:
                        continue
                    if len(parts) < 4:
                        raise ValueError("%s:%d has %d fields, expected at least 4" % (path, no, len(parts)))
                    ids, fill = np.zeros((len(self.FIELDS), L), np.int64), [0] * len(self.FIELDS)
                    for elem in parts[4:]:
                        field, _, feat = elem.strip().partition(":")
                        i = self.index.get(field)
                        if i is None:
                            continue
                        if fill[i] < L:
                            ids[i, fill[i]] = int(feat)
                        fill[i] += 1
                    yield ids, int(parts[1]), int(parts[2])

    def __iter__(self):
        group = []
        for row in self._rows():
            group.append(row)
            if len(group) == self.batch_size:
                ids = torch.from_numpy(np.stack([r[0] for r in group]))
                click = torch.tensor([r[1] for r in group], dtype=torch.int64)
                buy = torch.tensor([r[2] for r in group], dtype=torch.int64)
                group = []
                yield tuple(t.to(self.device, non_blocking=True) for t in (ids, click, buy))


class AitmReader:
    """models/multitask/aitm/aitm_reader.py RecDataset with the batching of the other readers (drop_last).  As the reference,
    it reads ONLY file_list[0] and skips that file's first line, the header `click,purchase,<18 feature names>`; every other
    line is comma-separated integers: click, purchase, then one id per field in the header's (= the config's) order.  Yields
    (ids [B, F] i64, click [B] i64, buy [B] i64) on `device`: ids[:, f] is the reference's f-th feature tensor."""

    def __init__(self, file_list, batch_size, device="cuda"):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        self.feature_names = []

    def _rows(self):
        path = self.file_list[0]
        with open(path, "r") as f:
            self.feature_names = f.readline().strip().split(",")[2:]
            for no, line in enumerate(f, 2):
                parts = line.strip().split(",")
                if parts == [""]:
                    continue
                vals = [int(v) for v in parts]
                if len(vals) != 2 + len(self.feature_names):
                    raise ValueError("%s:%d has %d fields, expected %d" % (path, no, len(vals), 2 + len(self.feature_names)))
                yield vals

    def __iter__(self):
        group = []
        for row in self._rows():
            group.append(row)
            if len(group) == self.batch_size:
                a = torch.tensor(group, dtype=torch.int64)
                group = []
                yield tuple(t.contiguous().to(self.device, non_blocking=True) for t in (a[:, 2:], a[:, 0], a[:, 1]))


class MindReader:
    """models/recall/mind/mind_reader.py RecDataset with the batching of the other readers (drop_last).  Lines are
    `user,item,timestamp`; a user's items are sorted by timestamp (a stable sort: ties keep file order).  An epoch draws
    batch_size users at a time with random.sample until batches_per_epoch * batch_size samples have been yielded; a user
    with at most 4 items is skipped; the cut position k is random.choice(range(4, len)) after random.seed(12345) — the
    reference reseeds before EVERY choice, so k depends only on the history's length, and so does the stream that the next
    random.sample continues from.  The history is the maxlen items before k (fewer: padded with 0 behind them).  Yields
    (hist_item [B, maxlen] i64, target_item [B, 1] i64, seq_len [B, 1] i64) on `device`."""

    def __init__(self, file_list, batch_size, device="cuda", maxlen=30, batches_per_epoch=1000):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        self.maxlen, self.batches_per_epoch = int(maxlen), int(batches_per_epoch)
        self.count = 0
        self.graph, users, items = {}, set(), set()
        for path in self.file_list:
            with open(path, "r") as f:
                for line in f:
                    conts = line.strip().split(",")
                    user_id, item_id, time_stamp = int(conts[0]), int(conts[1]), int(conts[2])
                    users.add(user_id)
                    items.add(item_id)
                    self.graph.setdefault(user_id, []).append((item_id, time_stamp))
        for user_id, value in self.graph.items():
            value.sort(key=lambda x: x[1])
            self.graph[user_id] = [x[0] for x in value]
        self.users, self.items = list(users), list(items)

    def samples(self):
        """The reference's __iter__: one (hist_item [maxlen], target_item [1], seq_len [1]) int64 triple per sample."""
        import random
        random.seed(12345)
        while True:
            user_id_list = random.sample(self.users, self.batch_size)
            if self.count >= self.batches_per_epoch * self.batch_size:
                self.count = 0
                break
            for user_id in user_id_list:
                item_list = self.graph[user_id]
                if len(item_list) <= 4:
                    continue
                random.seed(12345)
                k = random.choice(range(4, len(item_list)))
                item_id = item_list[k]
                if k >= self.maxlen:
                    hist_item_list = item_list[k - self.maxlen:k]
                    hist_item_len = len(hist_item_list)
                else:
                    hist_item_list = item_list[:k] + [0] * (self.maxlen - k)
                    hist_item_len = k
                self.count += 1
                yield [np.array(hist_item_list).astype("int64"), np.array([item_id]).astype("int64"),
                       np.array([hist_item_len]).astype("int64")]

    def __iter__(self):
        group = []
        for s in self.samples():
            group.append(s)
            if len(group) == self.batch_size:
                cols = [torch.from_numpy(np.stack([g[i] for g in group])) for i in range(3)]
                group = []
                yield tuple(t.contiguous().to(self.device, non_blocking=True) for t in cols)


class MindInferReader:
    """models/recall/mind/mind_infer_reader.py RecDataset with the batching of the other readers (drop_last).  Lines are
    space-separated `slot:feasign` pairs of the slots hist_item and eval_item.  The history keeps its LAST maxlen items, the
    evaluation list its FIRST maxlen, both padded with 0 behind; a line without an eval_item is skipped.  Yields
    (hist_item [B, maxlen] i64, seq_len [B, 1] i64, eval_items [B, 1, maxlen] i64): the first two on `device`, the last on
    the host, where the retrieval metrics are counted."""

    def __init__(self, file_list, batch_size, device="cuda", maxlen=30):
        self.file_list, self.batch_size, self.device, self.maxlen = list(file_list), int(batch_size), device, int(maxlen)
        self.slots = "hist_item eval_item".split(" ")
        self.padding = 0

    def samples(self):
        """The reference's __iter__: [hist_item [maxlen], seq_len [1], eval_items [1, maxlen]] int64 per line."""
        slot2index = {s: i for i, s in enumerate(self.slots)}
        for path in self.file_list:
            with open(path, "r") as rf:
                for line in rf:
                    output = [(i, []) for i in self.slots]
                    for i in line.strip().split(" "):
                        slot_feasign = i.split(":")
                        if slot_feasign[0] not in self.slots:
                            continue
                        output[slot2index[slot_feasign[0]]][1].append(int(slot_feasign[1]))
                    output_list, seq_lens, eval_list = [], [], []
                    for key, value in output:
                        if key == "hist_item":
                            seq_lens.append(min(self.maxlen, len(value)))
                            value = value[-self.maxlen:] + [self.padding] * max(0, self.maxlen - len(value))
                        if key == "eval_item":
                            value = value[:self.maxlen] + [self.padding] * max(0, self.maxlen - len(value))
                            eval_list.append(value)
                            continue
                        output_list.append(np.array(value).astype("int64"))
                    if len(eval_list) == 0:
                        continue
                    yield output_list + [np.array(seq_lens).astype("int64")] + [np.array(eval_list).astype("int64")]

    def __iter__(self):
        group = []
        for s in self.samples():
            group.append(s)
            if len(group) == self.batch_size:
                cols = [torch.from_numpy(np.stack([g[i] for g in group])) for i in range(3)]
                group = []
                yield (cols[0].contiguous().to(self.device, non_blocking=True),
                       cols[1].contiguous().to(self.device, non_blocking=True), cols[2])


class Word2vecReader:
    """models/recall/word2vec/word2vec_reader.py RecDataset (with_shuffle_batch False) with the batching of the other readers
    (drop_last).  A line is a sentence of word ids; every word is paired with each word of its window.  The window is ONE
    draw made at construction — np.random.seed(12345); np.random.randint(1, window_size + 1) (word2vec_reader.py:60-61): 3 for
    window_size 5 — used for every word.  The negatives are cs.searchsorted of neg_num random.random() draws, cs the cumulative
    0.75-power unigram distribution of word_count_dict_path's counts; random.seed(12345) runs before EVERY sample's draws
    (word2vec_reader.py:113-116), so every sample gets the SAME neg_num ids.  Yields (in_ids [B] i64, target_ids [B, 1 + neg]
    i64, the true word first) on `device`: one tensor, so the step has no concat."""

    def __init__(self, file_list, batch_size, device="cuda", word_count_dict_path=None, window_size=5, neg_num=5):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        self.window_size, self.neg_num = int(window_size), int(neg_num)
        np.random.seed(12345)
        self.window = int(np.random.randint(1, self.window_size + 1))
        id_counts = []
        with open(word_count_dict_path, "r", encoding="utf-8") as f:
            for line in f:
                id_counts.append(int(line.split()[1]))
        word_all_count = sum(id_counts)
        np_power = np.power(np.array([float(count) / word_all_count for count in id_counts]), 0.75)
        self.cs = np.array(np_power / np_power.sum()).cumsum()

    def negatives(self):
        """The neg_num ids every sample gets."""
        import random
        random.seed(12345)
        return self.cs.searchsorted([random.random() for _ in range(self.neg_num)]).astype("int64")

    def samples(self):
        """The reference's __iter__: (input word, true word, negatives [neg_num]) per (word, context word) pair."""
        for path in self.file_list:
            with open(path, "r") as rf:
                for line in rf:
                    words = line.split()
                    for idx, target_id in enumerate(words):
                        start = max(idx - self.window, 0)
                        for context_id in words[start:idx] + words[idx + 1:idx + self.window + 1]:
                            yield int(target_id), int(context_id), self.negatives()

    def __iter__(self):
        ins, tgt = [], []
        for w, c, neg in self.samples():
            ins.append(w)
            tgt.append(np.concatenate([[c], neg]))
            if len(ins) == self.batch_size:
                a, b = torch.from_numpy(np.asarray(ins, np.int64)), torch.from_numpy(np.stack(tgt).astype(np.int64))
                ins, tgt = [], []
                yield a.to(self.device, non_blocking=True), b.contiguous().to(self.device, non_blocking=True)


class Word2vecInferReader:
    """models/recall/word2vec/word2vec_infer_reader.py RecDataset with drop_last batching.  A line is four words `a b c d`
    (lower-cased; a word missing from word_id_dict_path becomes <UNK>); reading STOPS at the first line that holds a ':'
    (word2vec_infer_reader.py:88-89).  Yields (a [B, 1], b [B, 1], c [B, 1], label [B, 1] i64 on `device`, inputs_word
    [B, 3] i64 on the host, where the first-that-is-no-input rule runs)."""

    def __init__(self, file_list, batch_size, device="cuda", word_id_dict_path=None):
        self.file_list, self.batch_size, self.device = list(file_list), int(batch_size), device
        self.word_to_id, self.id_to_word = {}, {}
        with open(word_id_dict_path, "r", encoding="utf-8") as f:
            for line in f:
                self.word_to_id[line.split(" ")[0]] = int(line.split(" ")[1])
                self.id_to_word[int(line.split(" ")[1])] = line.split(" ")[0]
        self.dict_size = len(self.word_to_id)

    def samples(self):
        for path in self.file_list:
            with open(path, "r") as rf:
                for line in rf:
                    if ":" in line:
                        return
                    features = [w if w in self.word_to_id else "<UNK>" for w in line.lower().split()]
                    ids = [self.word_to_id[features[i]] for i in range(4)]
                    yield [np.array([i]).astype("int64") for i in ids] + [np.array(ids[:3]).astype("int64")]

    def __iter__(self):
        group = []
        for s in self.samples():
            group.append(s)
            if len(group) == self.batch_size:
                cols = [torch.from_numpy(np.stack([g[i] for g in group])) for i in range(5)]
                group = []
                yield tuple(t.contiguous().to(self.device, non_blocking=True) for t in cols[:4]) + (cols[4],)


# ---------------------------------------------------------------------------------------------------- TiSASRec (MovieLens)
def tisas_compute_repos(time_seq, time_span):
    """movielens_reader.py:123-133 computeRePos, vectorised: |t_i - t_j| clipped to time_span -> int64 [n, n]."""
    t = np.asarray(time_seq, np.int64)
    return np.minimum(np.abs(t[:, None] - t[None, :]), int(time_span)).astype(np.int64)


def tisas_time_slice(time_set):
    time_min = min(time_set)
    return {t: int(round(float(t - time_min))) for t in time_set}


def tisas_clean_and_sort(User, time_map):
    """movielens_reader.py:157-196 cleanAndsort, statement for statement: users and items are numbered in the iteration
    order of a Python set, every user's times are rescaled by the user's own smallest non-zero gap."""
    User_filted, user_set, item_set = dict(), set(), set()
    for user, items in User.items():
        user_set.add(user)
        User_filted[user] = items
        for item in items:
            item_set.add(item[0])
    user_map, item_map = dict(), dict()
    for u, user in enumerate(user_set):
        user_map[user] = u + 1
    for i, item in enumerate(item_set):
        item_map[item] = i + 1
    for user, items in User_filted.items():
        User_filted[user] = sorted(items, key=lambda x: x[1])
    User_res = dict()
    for user, items in User_filted.items():
        User_res[user_map[user]] = list(map(lambda x: [item_map[x[0]], time_map[x[1]]], items))
    time_max = set()
    for user, items in User_res.items():
        time_list = list(map(lambda x: x[1], items))
        time_diff = set()
        for i in range(len(time_list) - 1):
            if time_list[i + 1] - time_list[i] != 0:
                time_diff.add(time_list[i + 1] - time_list[i])
        time_scale = 1 if len(time_diff) == 0 else min(time_diff)
        time_min = min(time_list)
        User_res[user] = list(map(lambda x: [x[0], int(round((x[1] - time_min) / time_scale) + 1)], items))
        time_max.add(max(set(map(lambda x: x[1], User_res[user]))))
    return User_res, len(user_set), len(item_set), max(time_max), user_map, item_map


def tisas_data_partition(fname):
    """movielens_reader.py:199-249 data_partition: lines of 4 (user, item, rating, time) or 3 (user, item, time) tab-separated
    columns; users and items with fewer than 5 events are dropped; the last two events of a user with at least 3 are the
    valid and the test item.  -> (user_train, user_valid, user_test, usernum, itemnum, timenum, user_map, item_map)."""
    from collections import defaultdict
    User, user_count, item_count, time_set = defaultdict(list), defaultdict(int), defaultdict(int), set()

    def rows():
        with open(fname, "r") as f:
            for line in f:
                cols = line.rstrip().split("\t")
                if len(cols) == 4:
                    u, i, _, ts = cols
                else:
                    u, i, ts = cols
                yield int(u), int(i), ts

    for u, i, _ in rows():
        user_count[u] += 1
        item_count[i] += 1
    for u, i, ts in rows():
        ts = float(ts)
        if user_count[u] < 5 or item_count[i] < 5:
            continue
        time_set.add(ts)
        User[u].append([i, ts])
    User, usernum, itemnum, timenum, user_map, item_map = tisas_clean_and_sort(User, tisas_time_slice(time_set))
    user_train, user_valid, user_test = {}, {}, {}
    for user in User:
        if len(User[user]) < 3:
            user_train[user], user_valid[user], user_test[user] = User[user], [], []
        else:
            user_train[user], user_valid[user], user_test[user] = User[user][:-2], [User[user][-2]], [User[user][-1]]
    return user_train, user_valid, user_test, usernum, itemnum, timenum, user_map, item_map


class TisasDataset:
    """models/recall/tisas/movielens_reader.py RecDataset, a map-style dataset.  mode "train": __getitem__ IGNORES its index
    and draws the user and the negatives from the generator seeded 2021 in the constructor (the reference seeds the global
    np.random; a RandomState of the same seed yields the same draws) -> (seq [L], time_matrix [L, L], pos [L], neg [L]);
    mode "test": (seq [L], time_matrix [L, L], item_idx [101]) of test user idx, the test item first, then 100 sampled
    negatives.  All int64."""

    def __init__(self, file_list, maxlen, time_span, mode="test"):
        self.rng = np.random.RandomState(2021)
        (self.user_train, self.user_valid, self.user_test, self.usernum, self.itemnum, self.timenum, self.user_map,
         self.item_map) = tisas_data_partition(list(file_list)[0])
        self.maxlen, self.time_span, self.mode = int(maxlen), int(time_span), mode
        self.relation_matrix = {}
        for user in range(1, self.usernum + 1):                 # Relation(): the matrix of user_train[:-1]
            time_seq = np.zeros([self.maxlen], dtype=np.int64)
            idx = self.maxlen - 1
            for i in reversed(self.user_train[user][:-1]):
                time_seq[idx] = i[1]
                idx -= 1
                if idx == -1:
                    break
            self.relation_matrix[user] = tisas_compute_repos(time_seq, self.time_span)
        if self.mode == "test":
            if self.usernum > 10000:
                raise ValueError("TiSASRec test reader: more than 10000 users — the reference samples them with "
                                 "np.random.sample(user_idx, 10000), a call that takes no second argument and cannot run "
                                 "(movielens_reader.py:45-46); this branch has no behaviour to mirror")
            self.test_users = [u for u in range(1, self.usernum + 1) if len(self.user_train[u]) > 0]

    def __len__(self):
        return len(self.user_train) if self.mode == "train" else len(self.test_users)

    def _random_neq(self, lo, hi, s):
        t = self.rng.randint(lo, hi)
        while t in s:
            t = self.rng.randint(lo, hi)
        return t

    def sample(self, user):
        L = self.maxlen
        seq, time_seq, pos, neg = (np.zeros([L], dtype=np.int64) for _ in range(4))
        nxt = self.user_train[user][-1][0]
        idx = L - 1
        ts = set(map(lambda x: x[0], self.user_train[user]))
        for i in reversed(self.user_train[user][:-1]):
            seq[idx], time_seq[idx], pos[idx] = i[0], i[1], nxt
            if nxt != 0:
                neg[idx] = self._random_neq(1, self.itemnum + 1, ts)
            nxt = i[0]
            idx -= 1
            if idx == -1:
                break
        return seq, self.relation_matrix[user].astype("int64"), pos, neg

    def __getitem__(self, idx):
        if self.mode == "train":
            user = self.rng.randint(1, self.usernum + 1)
            while len(self.user_train[user]) <= 1:
                user = self.rng.randint(1, self.usernum + 1)
            return self.sample(user)
        u = self.test_users[idx]
        L = self.maxlen
        seq, time_seq = np.zeros([L], dtype=np.int64), np.zeros([L], dtype=np.int64)
        idx = L - 1
        seq[idx], time_seq[idx] = self.user_valid[u][0][0], self.user_valid[u][0][1]
        idx -= 1
        for i in reversed(self.user_train[u]):
            seq[idx], time_seq[idx] = i[0], i[1]
            idx -= 1
            if idx == -1:
                break
        time_matrix = tisas_compute_repos(time_seq, self.time_span)
        item_idx = [self.user_test[u][0][0]]
        rated = set(map(lambda x: x[0], self.user_train[u]))
        rated.add(self.user_valid[u][0][0])
        rated.add(0)
        for _ in range(100):
            t = self.rng.randint(1, self.itemnum + 1)
            while t in rated:
                t = self.rng.randint(1, self.itemnum + 1)
            item_idx.append(t)
        return seq, time_matrix, np.array(item_idx, dtype=np.int64)


class TisasReader:
    """The reference's DataLoader over a TisasDataset: indices 0 .. len - 1 in order, batch_size samples stacked, the last
    partial batch dropped.  ONE dataset serves every epoch (the generator's draws carry on, as in the reference).  Yields
    tuples of int64 tensors on `device`."""

    def __init__(self, file_list, batch_size, device="cuda", maxlen=50, time_span=256, mode="train"):
        self.dataset = TisasDataset(file_list, maxlen, time_span, mode)
        self.batch_size, self.device = int(batch_size), device

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def __iter__(self):
        for b in range(len(self)):
            rows = [self.dataset[b * self.batch_size + j] for j in range(self.batch_size)]
            yield tuple(torch.from_numpy(np.stack([r[c] for r in rows])).contiguous().to(self.device, non_blocking=True)
                        for c in range(len(rows[0])))


# ------------------------------------------------------------------ ENSFM (models/recall/ensfm/movielens_reader.py)
class EnsfmDataset:
    """LoadData + RecDataset of the reference's movielens_reader.py over <data_root>/train.csv and test.csv, whose lines are
    `<user features joined by '-'>,<item features joined by '-'>`.  No scipy: the reference's two csr_matrix user-item
    sets (Train_data, Test_data) are kept as plain (user id, item id) arrays, which is all infer.py reads of them.

      * user_field_M / item_field_M: the largest feature id of TRAIN + 1 (movielens_reader.py:75-97);
      * items, then users, are numbered in order of first appearance over train.csv then test.csv (:99-157);
      * item_map_list [I + 1, Fi]: every item's features in id order, then item 0's features AGAIN as row I, the padding item
        (:60-68);
      * user_train [U, Fu] / item_train [U, P]: one row per user with train positives in order of first appearance, the
        positives in file order, padded with I to the longest list (:184-198);
      * user_test [n_test_lines, Fu]: the user features of EVERY test line, duplicates included (:227-229).
    __getitem__ as the reference: train -> (user_train[i], item_map_list, item_train[i], I), test -> (user_test[i],
    item_map_list)."""

    def __init__(self, file_list, mode="train"):
        root = os.path.dirname(file_list[0]) if not os.path.isdir(file_list[0]) else file_list[0]
        self.trainfile, self.testfile = os.path.join(root, "train.csv"), os.path.join(root, "test.csv")
        self.mode = mode
        rows = {f: self._read(f) for f in (self.trainfile, self.testfile)}
        tr = rows[self.trainfile]
        self.user_field_M = max(max(int(x) for x in u.split("-")) for u, _ in tr) + 1
        self.item_field_M = max(max(int(x) for x in i.split("-")) for _, i in tr) + 1
        self.binded_items, self.binded_users = {}, {}
        for col, table in ((1, self.binded_items), (0, self.binded_users)):
            for f in (self.trainfile, self.testfile):
                for r in rows[f]:
                    if r[col] not in table:
                        table[r[col]] = len(table)
        self.item_bind_M, self.user_bind_M = len(self.binded_items), len(self.binded_users)
        feats = lambda key: [int(x) for x in key.strip().split("-")]
        items = sorted(self.binded_items, key=self.binded_items.get)
        # movielens_reader.py:66-68: item 0's features again, as the row of the padding id I
        self.item_map_list = np.asarray([feats(k) for k in items] + [feats(items[0])], np.int64)
        positives = {}
        for u, i in tr:
            positives.setdefault(self.binded_users[u], []).append(self.binded_items[i])
        self.max_positive_len = max(len(v) for v in positives.values())
        users = sorted(self.binded_users, key=self.binded_users.get)
        self.user_train = np.asarray([feats(users[uid]) for uid in positives], np.int64)
        self.item_train = np.full((len(positives), self.max_positive_len), self.item_bind_M, np.int64)
        for r, lst in enumerate(positives.values()):
            self.item_train[r, :len(lst)] = lst
        self.user_test = np.asarray([feats(u) for u, _ in rows[self.testfile]], np.int64)
        pairs = lambda rs: np.asarray(sorted({(self.binded_users[u], self.binded_items[i]) for u, i in rs}), np.int64).reshape(-1, 2)
        self.train_pairs, self.test_pairs = pairs(tr), pairs(rows[self.testfile])     # the non-zeros of Train_data / Test_data
        self._masks = None

    @staticmethod
    def _read(path):
        with open(path) as f:
            return [tuple(ln.strip().split(",")[:2]) for ln in f if ln.strip()]

    def __len__(self):
        return len(self.user_train) if self.mode == "train" else len(self.user_test)

    def __getitem__(self, idx):
        if self.mode == "train":
            return self.user_train[idx], self.item_map_list, self.item_train[idx], np.asarray(self.item_bind_M)
        return self.user_test[idx], self.item_map_list

    def user_ids(self, user_features):
        """infer.py:186-189: rows of user features -> bound user ids."""
        return [self.binded_users["-".join(str(int(x)) for x in row)] for row in np.asarray(user_features)]

    def user_masks(self, user_features, device, user_ids=None):
        """(train_mask, test_mask) bool [B, I] of the users behind rows of user features: infer.py's
        Train_data[user_id].nonzero() and Test_data[user_id].nonzero().  user_ids (int64 [B] on `device`, from EnsfmReader):
        the rows' bound ids, so nothing comes back to the host; None: they are looked up from the feature rows."""
        if self._masks is None or self._masks[0].device != torch.empty(0, device=device).device:
            dense = []
            for pr in (self.train_pairs, self.test_pairs):
                m = torch.zeros(self.user_bind_M, self.item_bind_M, dtype=torch.bool)
                m[torch.from_numpy(pr[:, 0]), torch.from_numpy(pr[:, 1])] = True
                dense.append(m.to(device))
            self._masks = dense
        if user_ids is None:
            user_ids = torch.as_tensor(self.user_ids(user_features.cpu().numpy() if torch.is_tensor(user_features) else user_features),
                                       dtype=torch.int64, device=self._masks[0].device)
        return self._masks[0][user_ids], self._masks[1][user_ids]


class EnsfmReader:
    """The reference's DataLoader over an EnsfmDataset: indices in order, batch_size samples stacked, the last partial batch
    dropped.  The item attribute matrix goes to the device ONCE; every batch carries the same tensor behind a leading axis of
    length 1 (the reference stacks B copies and create_feeds takes copy 0: dygraph_model.py:33-35)."""

    def __init__(self, file_list, batch_size, device="cuda", mode="train"):
        self.dataset = EnsfmDataset(file_list, mode)
        self.batch_size, self.device = int(batch_size), device
        self.item_attribute = torch.from_numpy(self.dataset.item_map_list).contiguous().to(device)
        self.item_bind_M = torch.full((1,), self.dataset.item_bind_M, dtype=torch.int64)      # a host scalar: it stays there
        self.test_user_ids = None
        if mode != "train":                                   # the bound id of every test line, on the device once
            self.test_user_ids = torch.as_tensor(self.dataset.user_ids(self.dataset.user_test), dtype=torch.int64).to(device)

    def __len__(self):
        return len(self.dataset) // self.batch_size

    def __iter__(self):
        d, bs = self.dataset, self.batch_size
        for b in range(len(self)):
            sl = slice(b * bs, (b + 1) * bs)
            if d.mode == "train":
                yield (torch.from_numpy(d.user_train[sl]).contiguous().to(self.device, non_blocking=True),
                       self.item_attribute[None], torch.from_numpy(d.item_train[sl]).contiguous().to(self.device, non_blocking=True),
                       self.item_bind_M)
            else:
                yield (torch.from_numpy(d.user_test[sl]).contiguous().to(self.device, non_blocking=True), self.item_attribute[None],
                       self.test_user_ids[sl])


def ncf_parse(file_list):
    """ncf/movielens_reader.py:26-39: every line `user,item,label`, all int -> three int64 arrays in file order."""
    cols = ([], [], [])
    for path in file_list:
        with open(path, "r") as rf:
            for line in rf:
                features = line.strip().split(",")
                for c in range(3):
                    cols[c].append(int(features[c]))
    return tuple(np.asarray(c, dtype=np.int64) for c in cols)


class NcfReader:
    """The reference's DataLoader over ncf/movielens_reader.py: the lines in file order, batch_size at a time, the last batch
    short when the lines do not divide (an IterableDataset's DataLoader does not drop it).  The three columns go to the device
    once; a batch is three [b, 1] int64 views."""

    def __init__(self, file_list, batch_size, device="cuda"):
        self.batch_size = int(batch_size)
        self.users, self.items, self.labels = (torch.from_numpy(c).to(device) for c in ncf_parse(file_list))

    def __len__(self):
        return -(-self.users.numel() // self.batch_size)

    def __iter__(self):
        for b in range(len(self)):
            sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
            yield self.users[sl].view(-1, 1), self.items[sl].view(-1, 1), self.labels[sl].view(-1, 1)


def dssm_parse(file_list, fields=None):
    """dssm/bq_reader_train.py:26-48 (fields=None: every field of a line) and bq_reader_infer.py (fields=2): a line is
    tab-separated fields, a field a comma-separated float vector -> one list of float32 arrays per line, in file order."""
    out = []
    for path in file_list:
        with open(path, "r") as rf:
            for line in rf:
                features = line.rstrip("\n").split("\t")
                out.append([np.array([float(x) for x in f.split(",")]).astype("float32")
                            for f in (features if fields is None else features[:fields])])
    return out


def dssm_csr(rows):
    """Dense float32 vectors -> CSR (cols int64, vals float32, lod int64 [len(rows) + 1], row_of int32): exact zeros are
    dropped, nothing else is, and a value other than 1.0 is kept."""
    nz = [np.flatnonzero(r) for r in rows]
    lod = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in nz], out=lod[1:])
    cols = np.concatenate(nz).astype(np.int64) if nz else np.zeros(0, np.int64)
    vals = np.concatenate([r[c] for r, c in zip(rows, nz)]).astype(np.float32) if nz else np.zeros(0, np.float32)
    row_of = np.repeat(np.arange(len(rows), dtype=np.int32), np.diff(lod))
    return cols, vals, lod, row_of


def dssm_group(cols, width):
    """The entries of a CSR input grouped by column, on the host, as rec_ids_group(cols, num_rows=width) writes them on the
    device: sorted_pos int32 [nnz] (entry indices, stably sorted by column), uniq_rows int64 [nnz] (the first U: the distinct
    columns, ascending), seg_offset int32 [nnz + 1] (sorted_pos[seg_offset[u] : seg_offset[u + 1]] belong to uniq_rows[u]),
    n_uniq int32 [4] = {U, entries kept, 0, 0}.  A column outside [0, width) is dropped.  A batch that carries these spares
    its train step the device sort."""
    cols = np.asarray(cols, np.int64)
    n = len(cols)
    keep = np.flatnonzero((cols >= 0) & (cols < width))
    order = keep[np.argsort(cols[keep], kind="stable")]
    uniq, counts = np.unique(cols[keep], return_counts=True)
    sorted_pos, uniq_rows, seg_offset = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(n + 1, np.int32)
    sorted_pos[:len(order)], uniq_rows[:len(uniq)] = order, uniq
    np.cumsum(counts, out=seg_offset[1:len(uniq) + 1])
    return sorted_pos, uniq_rows, seg_offset, np.asarray([len(uniq), len(keep), 0, 0], np.int32)


class DssmReader:
    """The reference's DataLoader over dssm/bq_reader_train.py (mode "train": every field — query, positive, negatives) or
    bq_reader_infer.py (mode "infer": the first two): the lines in file order, batch_size at a time, the last batch short.
    A batch is [query, docs] in CSR — each (cols, vals, lod, row_of) followed by dssm_group's four arrays, on the device, docs
    holding the batch's positives first and then each negative field's rows — or, with dense=True, the reference's list of
    [b, trigram_d] float32 tensors."""

    def __init__(self, file_list, batch_size, device="cuda", mode="train", dense=False):
        self.batch_size, self.device, self.dense = int(batch_size), device, dense
        self.lines = dssm_parse(file_list, None if mode == "train" else 2)
        if len({len(l) for l in self.lines}) > 1 or (self.lines and len(self.lines[0]) < 2):
            raise ValueError("dssm: every line needs the same number of fields, at least a query and a positive document")

    def __len__(self):
        return -(-len(self.lines) // self.batch_size)

    def __iter__(self):
        for b in range(len(self)):
            lines = self.lines[b * self.batch_size:(b + 1) * self.batch_size]
            fields = [[l[f] for l in lines] for f in range(len(lines[0]))]
            if self.dense:
                yield [torch.from_numpy(np.stack(f)).to(self.device) for f in fields]
            else:
                out = []
                for rows in (fields[0], [r for f in fields[1:] for r in f]):
                    csr = dssm_csr(rows)
                    out.append(tuple(torch.from_numpy(a).to(self.device) for a in csr + dssm_group(csr[0], len(rows[0]))))
                yield out


def letor_parse(file_list):
    """The parse of match-pyramid/letor_reader.py: a line holds the left and the right sentence, tab-separated, each a
    comma-separated list of word ids -> (left, right) int64 [lines, Ll] / [lines, Lr], in file order.  Every line must hold the
    same two lengths (the reference's DataLoader stacks them)."""
    sentences = ([], [])
    for path in file_list:
        with open(path) as f:
            for line in f:
                for side, text in zip(sentences, line.rstrip("\n").split("\t")[:2]):
                    side.append(np.array(text.split(","), dtype=np.int64))
    if any(len({len(x) for x in side}) > 1 for side in sentences) or len(sentences[0]) != len(sentences[1]):
        raise ValueError("match-pyramid: every line needs two sentences of the same sentence lengths")
    if not sentences[0]:
        return np.zeros((0, 0), np.int64), np.zeros((0, 0), np.int64)
    return np.stack(sentences[0]), np.stack(sentences[1])


class LetorReader:
    """The reference's DataLoader over match-pyramid/letor_reader.py: the lines in file order, batch_size at a time, the last
    batch short.  A batch is [sentence_left int64 [b, Ll], sentence_right int64 [b, Lr]] on the device."""

    def __init__(self, file_list, batch_size, device="cuda"):
        self.batch_size, self.device = int(batch_size), device
        left, right = letor_parse(file_list)
        self.left, self.right = torch.from_numpy(left).to(device), torch.from_numpy(right).to(device)

    def __len__(self):
        return -(-self.left.shape[0] // self.batch_size)

    def __iter__(self):
        for b in range(len(self)):
            sl = slice(b * self.batch_size, (b + 1) * self.batch_size)
            yield [self.left[sl], self.right[sl]]
