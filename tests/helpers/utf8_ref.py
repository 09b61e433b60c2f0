"""The decode rule of latok_utf8_decode_batch (include/latok_hip.h, latok_amd/csrc/utf8_decode.h) restated in plain Python, twice:
a scalar loop that is meant to be obviously right, and a numpy form for streams of several MB.  Both read the PACKED byte stream
of a batch:

* lead(i) := (u8[i] & 0xC0) != 0x80; there is one code point per lead byte, total_cps = number of leads;
* a lead b0 needs k continuation bytes: k = 0 below 0x80, 1 for 0xC0..0xDF, 2 for 0xE0..0xEF, 3 for 0xF0..0xFF (0xF8..0xFF carry
  3 payload bits like 0xF0..0xF7);
* if bytes i+1 .. i+k all exist in the batch and are 10xxxxxx the value is the payload bits put together -- nothing is refused as
  overlong, surrogate or above U+10FFFF -- otherwise it is U+FFFD;
* cp_row_off[s] = number of leads in [0, byte_off[s]).

The window of a lead is read from the packed stream: it runs over its string's end into the next string, never past the batch.
Nothing here is derived from the code under test."""
import numpy as np

REPLACEMENT = 0xFFFD


def is_lead(b):
    return (b & 0xC0) != 0x80


def n_cont(b0):
    """continuation bytes the lead byte b0 announces"""
    return 0 if b0 < 0x80 else 1 if b0 < 0xE0 else 2 if b0 < 0xF0 else 3


def cp_at(data, i):
    """code point of the lead byte data[i]"""
    b0 = data[i]
    k = n_cont(b0)
    if k == 0:
        return b0
    tail = data[i + 1:i + 1 + k]                       # shorter than k where the batch ends
    if len(tail) < k or any((b & 0xC0) != 0x80 for b in tail):
        return REPLACEMENT
    cp = b0 & (0x3F >> k)
    for b in tail:
        cp = (cp << 6) | (b & 0x3F)
    return cp


def decode_scalar(data):
    """bytes -> (code points, byte position of each), the scalar loop"""
    data = bytes(data)
    leads = [i for i, b in enumerate(data) if is_lead(b)]
    return [cp_at(data, i) for i in leads], leads


def decode_batch_scalar(data, byte_off):
    """-> (cps list, cp_row_off list, total_cps)"""
    cps, leads = decode_scalar(data)
    return cps, _rows_scalar(leads, byte_off), len(cps)


def _rows_scalar(leads, byte_off):
    """number of leads below each offset, one merge pass (offsets ascend)"""
    row, k = [], 0
    for o in byte_off:
        while k < len(leads) and leads[k] < int(o):
            k += 1
        row.append(k)
    return row


def decode_per_lead(u8):
    """uint8 array -> (cps uint32, byte position of every cp), the numpy form"""
    u8 = np.ascontiguousarray(u8, dtype=np.uint8)
    lead = np.flatnonzero((u8 & 0xC0) != 0x80)
    padded = np.concatenate([u8, np.full(3, 0xFF, np.uint8)])        # a byte that does not exist is no continuation byte
    b0 = padded[lead].astype(np.uint32)
    k = (b0 >= 0xC0).astype(np.uint32) + (b0 >= 0xE0) + (b0 >= 0xF0)
    cp = np.where(k == 0, b0, b0 & (np.uint32(0x3F) >> k))
    bad = np.zeros(lead.size, bool)
    for j in (1, 2, 3):
        nxt = padded[lead + j].astype(np.uint32)
        need = k >= j
        bad |= need & ((nxt & 0xC0) != 0x80)
        cp = np.where(need, (cp << np.uint32(6)) | (nxt & 0x3F), cp)
    cp[bad] = REPLACEMENT
    return cp.astype(np.uint32), lead


def decode_batch(u8, byte_off):
    """the full contract: -> (cps uint32[total_cps], cp_row_off int64[n_str + 1], total_cps)"""
    byte_off = np.asarray(byte_off, np.int64)
    total = int(byte_off[-1]) if byte_off.size > 1 else 0
    cps, lead = decode_per_lead(np.asarray(u8, np.uint8)[:total])
    row = np.searchsorted(lead, byte_off, side="left").astype(np.int64)
    return cps, row, int(cps.size)
