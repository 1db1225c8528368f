"""host-side readers of text columns in COLUMN chunk images (pg_strom_amd/kds.py): no GPU needed"""
import numpy as np

from pg_strom_amd import kds


def test_decode_text_column_reads_offset_header_payload():
    words = [b"", b"a", b"abc", b"x" * 126, b"x" * 127, b"\xff\x80" * 300, b"never"]
    isnull = np.array([0, 0, 0, 0, 0, 0, 1], dtype=bool)
    buf = kds.build_kds("column", [kds.Column("int4", np.arange(7, dtype=np.int32)), kds.Column("text", words, isnull)])
    assert kds.decode_text_column(buf, 1) == words[:6] + [None]
    # datums that are not plain come back whole, header included
    compressed = np.array([(20 << 2) | 2], dtype="<u4").tobytes() + b"\1" * 16
    external = bytes([0x01, 18]) + b"\2" * 16
    buf = kds.build_kds("column", [kds.Column("text_raw", [kds.varlena_datum(b"abc"), compressed, external])])
    assert kds.decode_text_column(buf, 0) == [b"abc", bytearray(compressed), bytearray(external)]


def test_column_type_tags():
    assert kds.column_type_oid("text") == 25
    assert kds.column_type_oid("character") == (0x10000 | 1042)        # STROM_BPCHARNOID
    assert kds.column_type_oid("char1") == 1042 and kds.column_type_oid("int8") == 20
