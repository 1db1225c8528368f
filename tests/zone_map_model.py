"""
An independent model of a COLUMN chunk's zone map (kern_coldir.stat_flags / minval / maxval,
include/strom_kds.h), and two readers of heap chunks, shared by test_zone_map_cpu.py and
test_ingest_edges_gpu.py.  Plain Python over Python values: nothing here calls the library
under test, so an error shared by the host builder and the device kernels does not pass.

    integer-like   flags 1     min / max of the not-NULL rows, as Python ints
    float4/float8  flags 1|2   NaN left out, compared as float64, stated as IEEE double bits
                               (the sign of a zero bound is not part of the contract)
    numeric        flags 4     floor(min), ceil(max) of the values (KDS_COLSTAT_INTPART);
                               no zone map when a value's integer part is beyond int64
    nothing to bound (all NULL, all NaN): flags 0
"""
import math
import struct
from decimal import Decimal

import numpy as np

MINMAX, ISFLOAT, INTPART = 1, 2, 4
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1

INTEGER_TYPES = ("bool", "char1", "int2", "int4", "int8", "date", "time", "timestamp", "decimal")
FLOAT_TYPES = ("float4", "float8")


def double_bits(x):
    """a Python float -> its IEEE double bits as a signed 64-bit integer (what minval / maxval hold)"""
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def bits_double(b):
    return struct.unpack("<d", struct.pack("<q", int(b)))[0]


def numeric_image_value(image):
    """64-bit device numeric (exponent 63..58 signed, sign 57, mantissa 56..0) -> Decimal"""
    image = int(image) & (2**64 - 1)
    exp = image >> 58
    exp = exp - 64 if exp >= 32 else exp
    d = Decimal(image & (2**57 - 1)).scaleb(exp)
    return -d if (image >> 57) & 1 else d


def expected(sqltype, values, isnull=None):
    """(stat_flags, minval, maxval) of a column of 'values' (Python / numpy scalars; Decimals for
    'numeric'), rows with isnull[i] left out.  minval / maxval are 0 where flags are 0."""
    if isinstance(values, np.ndarray):
        values = values.tolist()                        # Python ints / floats (float4 -> float8 is exact)
    if isnull is not None:
        values = [v for v, isn in zip(values, np.asarray(isnull).tolist()) if not isn]
    live = list(values)
    if sqltype in FLOAT_TYPES:
        live = [float(v) for v in live]
        live = [v for v in live if not math.isnan(v)]
        if not live:
            return (0, 0, 0)
        return (MINMAX | ISFLOAT, double_bits(min(live)), double_bits(max(live)))
    if sqltype == "numeric":
        if not live:
            return (0, 0, 0)
        lo = math.floor(min(Decimal(v) for v in live))
        hi = math.ceil(max(Decimal(v) for v in live))
        if lo < INT64_MIN or hi > INT64_MAX:            # some value's integer part is beyond int64
            return (0, 0, 0)
        return (INTPART, lo, hi)
    assert sqltype in INTEGER_TYPES, sqltype
    live = [int(v) for v in live]
    if not live:
        return (0, 0, 0)
    return (MINMAX, min(live), max(live))


def same(got, want):
    """do two (stat_flags, minval, maxval) state the same zone map?  Float bounds that are zero
    compare by value (-0.0 == 0.0), everything else bit for bit."""
    if got[0] != want[0]:
        return False
    if got[0] == 0:
        return True
    if got[0] & ISFLOAT:
        for g, w in zip(got[1:], want[1:]):
            if g != w and not (bits_double(g) == 0.0 and bits_double(w) == 0.0):
                return False
        return True
    return tuple(got[1:]) == tuple(want[1:])


def of_decoded(col):
    """the zone map a decoded COLUMN chunk's column states (kds.decode_column_chunk)"""
    if col["stat_flags"] == 0:
        return (0, 0, 0)
    return (col["stat_flags"], col["minval"], col["maxval"])


def content(col, sqltype):
    """(values, isnull) of a decoded COLUMN chunk's column as the model's inputs: what the
    chunk's own bytes say, whatever its directory claims"""
    raw = col["values"]
    isnull = None if col["notnull"] is None else ~col["notnull"]
    if sqltype == "float4":
        vals = raw.view(np.float32)
    elif sqltype == "float8":
        vals = raw.view(np.float64)
    elif sqltype == "numeric":
        vals = [numeric_image_value(x) for x in raw.view(np.uint64)]
    else:
        vals = raw
    return vals, isnull


# ---------------------------------------------------------------------
# heap chunks (KDS_FORMAT_ROW = 1, KDS_FORMAT_ROW_FLAT = 2)
# ---------------------------------------------------------------------
BLCKSZ = 8192


def _align(n, a):
    return (n + a - 1) & ~(a - 1)


def tuple_offsets(buf):
    """byte offset, from the chunk's head, of every row's heap tuple.
    ROW_FLAT: kern_rowitem.htup_offset.  ROW: kern_rowitem names a page and a 1-based line
    pointer; pages of 8192 bytes start, 8192-aligned, behind the row items; line pointers start
    24 bytes into a page and hold the tuple's offset within the page in their low 15 bits."""
    u32 = np.frombuffer(buf[:48].tobytes(), dtype="<u4")
    ncols, nitems, maxblocks = int(u32[4]), int(u32[5]), int(u32[8])
    fmt = int(buf[36])
    assert fmt in (1, 2)
    items_at = _align(48 + 8 * ncols, 16) + _align(16 * maxblocks, 16)
    items = np.frombuffer(buf[items_at:items_at + 4 * nitems].tobytes(), dtype="<u4")
    if fmt == 2:
        return [int(x) for x in items]
    pages_at = _align(items_at + _align(4 * nitems, 16), BLCKSZ)
    out = []
    for it in items:
        page = pages_at + BLCKSZ * (int(it) & 0xffff)
        lp_at = page + 24 + 4 * ((int(it) >> 16) - 1)
        lp = int(np.frombuffer(buf[lp_at:lp_at + 4].tobytes(), dtype="<u4")[0])
        out.append(page + (lp & 0x7fff))
    return out


def shorten_tuples(buf, rows, natts):
    """cut the tuples of 'rows' to natts[i] attributes each, in place: the low 11 bits of
    t_infomask2 (18 bytes into the tuple header) -- what ALTER TABLE ADD COLUMN leaves behind in
    the tuples written before it.  Attributes past a tuple's count read as NULL."""
    offs = tuple_offsets(buf)
    for r, k in zip(rows, natts):
        at = offs[int(r)] + 18
        word = int(buf[at]) | (int(buf[at + 1]) << 8)
        assert 0 < int(k) <= (word & 0x07ff)
        word = (word & ~0x07ff) | int(k)
        buf[at] = word & 0xff
        buf[at + 1] = word >> 8
