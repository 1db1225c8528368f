"""The union of key dictionaries (strom_keyunion_*) over the table of gpu_textdict_probe.py --
14-byte text keys in a COLUMN chunk -- for the record, all in one run, device events:
  (a) recode of the chunk's id column into the union's numbering   (median of 5 after one warm-up)
      next to what it replaces: encoding the source chunk again under the union dictionary, the
      steady-state probe + emit of gpu_textdict_probe.py (b)
  (b) one absorb of a dictionary, every key new: probe, ranks (count + offsets), settle, emit
      (median of 5 after one warm-up, a fresh union dictionary with a hint each time; then one
      absorb into a dictionary begun without a hint, and the absorb of keys that are all known)
No pass / fail rests on a time.
usage: gpu_keyunion_probe.py [rows] [distinct keys ...]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pg_strom_amd import kds, runtime
from pg_strom_amd.textdict import TextDictionary, recode

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
distincts = [int(float(a)) for a in sys.argv[2:]] or [100, 100_000, 1_000_000]
runtime.init()
PARTS = ("probe", "ranks", "settle", "emit", "rebuild")


def us(ns):
    return ns * 1e-3


def image_of(words):
    heap, offs = bytearray(), []
    for w in words:
        offs.append(len(heap))
        d = kds.varlena_datum(w)
        heap += d + b"\0" * (-len(d) % 4)
    return bytes(heap), np.array(offs, dtype=np.uint64)


for nd in distincts:
    rng = np.random.default_rng(1)
    pick = rng.integers(0, nd, n)
    t0 = time.perf_counter()
    otxt = [b"cust#%09d" % i for i in pick]
    outer = kds.build_kds("column", [kds.Column("text", otxt), kds.Column("int8", np.arange(n, dtype=np.int64))])
    print("== %d rows, %d distinct 14-byte keys; COLUMN chunk %.1f MB, built in %.1f s"
          % (n, nd, len(outer) / 1e6, time.perf_counter() - t0), flush=True)
    ds = runtime.DeviceStore.upload(outer)
    own = TextDictionary("text", nkeys_hint=nd)
    enc = own.encode(ds, [0], [1])
    nk = own.num_keys
    ids0 = kds.decode_column_chunk(enc.download())[0]["values"].copy()

    # the union: another shard's keys first (every second key, backwards), then this dictionary
    union = TextDictionary("text", nkeys_hint=nd)
    union.absorb(image_of([b"cust#%09d" % i for i in range(nd - 1, -1, -2)])).release()
    m = union.absorb_dict(own)
    k = union.union_kernel_ns()
    print("    union of %d + %d keys: %d keys; the absorb of this dictionary (%d new): probe %.1f ranks %.1f settle %.1f emit %.1f us"
          % ((nd + 1) // 2, nk, union.num_keys, union.num_keys - (nd + 1) // 2,
             us(k["probe"]), us(k["ranks"]), us(k["settle"]), us(k["emit"])), flush=True)
    mapping = m.ids()
    assert not np.array_equal(mapping, np.arange(nk))

    # (a) recode, and the alternative in the same run.  The map is a permutation-like injection into
    # [0, union.num_keys) and the union holds at least this dictionary's keys, so recoding the
    # recoded column again reads and writes the same amount: the first pass is checked, all are timed
    tr = []
    for it in range(6):
        recode(enc, [0], [m])
        if it == 0:
            assert np.array_equal(kds.decode_column_chunk(enc.download())[0]["values"], mapping[ids0])
        else:
            tr.append(us(union.union_kernel_ns()["recode"]))
        if union.num_keys > nk and it < 5:
            # ids beyond the map's size would be refused: back to this dictionary's own ids
            enc.release()
            enc = own.encode(ds, [0], [1])
    tp, te = [], []
    for it in range(6):
        again = union.encode(ds, [0], [1])
        kk = union.kernel_ns()
        if it:
            tp.append(us(kk["probe"]))
            te.append(us(kk["emit"]))
        if it == 5:
            assert np.array_equal(kds.decode_column_chunk(again.download())[0]["values"], mapping[ids0])
        again.release()
    r, p, e = np.median(tr), np.median(tp), np.median(te)
    print("(a) recode %8.1f us  %.2f Grows/s (min %.1f max %.1f)   |   encode again under the union: probe %8.1f + emit %6.1f = %8.1f us   recode / (probe + emit) = %.3f"
          % (r, n / r / 1e3, min(tr), max(tr), p, e, p + e, r / (p + e)), flush=True)
    m.release()
    union.release()

    # (b) absorb, every key new
    ts = {name: [] for name in PARTS}
    for it in range(6):
        g = TextDictionary("text", nkeys_hint=nk)
        g.absorb_dict(own).release()
        assert g.num_keys == nk
        kk = g.union_kernel_ns()
        if it:
            for name in PARTS:
                ts[name].append(us(kk[name]))
        if it == 5:
            g.absorb_dict(own).release()
            known = g.union_kernel_ns()
        g.release()
    med = {name: np.median(ts[name]) for name in PARTS}
    print("(b) absorb %d new keys (hint): probe %8.1f  ranks %6.1f  settle %7.1f  emit %6.1f  rebuild %6.1f us  = %8.1f us   (probe min %.1f max %.1f)"
          % (nk, med["probe"], med["ranks"], med["settle"], med["emit"], med["rebuild"], sum(med.values()),
             min(ts["probe"]), max(ts["probe"])), flush=True)
    print("(b) ... the same keys again, all known: probe %8.1f  ranks %6.1f  settle %7.1f  emit %6.1f us"
          % (us(known["probe"]), us(known["ranks"]), us(known["settle"]), us(known["emit"])), flush=True)
    g = TextDictionary("text")
    g.absorb_dict(own).release()
    kk = g.union_kernel_ns()
    print("(b) ... no hint (16 slots to begin with): probe %8.1f us (all probes of the call)  ranks %6.1f  settle %7.1f  emit %6.1f  rebuild %6.1f"
          % (us(kk["probe"]), us(kk["ranks"]), us(kk["settle"]), us(kk["emit"]), us(kk["rebuild"])), flush=True)
    g.release()
    enc.release()
    own.release()
    ds.release()
