"""Whole-batch entry points over the fused HIP kernel (additive to the reference surface).

A batch is CSR: ``cps`` = packed UTF-32 code points of all strings, ``row_off[n+1]`` = start of each string.
"""
import ctypes as C
import threading

import numpy as np

from . import _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def pack(texts):
    """list[str] -> (cps uint32[total], row_off int64[n+1])."""
    lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
    row_off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum(lens, out=row_off[1:])
    blob = "".join(texts).encode("utf-32-le", "surrogatepass")
    cps = np.frombuffer(blob, dtype="<u4").astype(np.uint32, copy=False)
    return np.ascontiguousarray(cps), row_off


def _csr(cps, row_off):
    cps = np.ascontiguousarray(cps, dtype=np.uint32)
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    if row_off.ndim != 1 or row_off.size < 1:
        raise ValueError("row_off must be a 1-D array of n_str + 1 offsets")
    if cps.ndim != 1 or (row_off.size > 1 and cps.size < int(row_off[-1])):
        raise ValueError("cps is shorter than row_off[-1]")
    return cps, row_off



class _Pinned:
    """keeps a pinned allocation alive for as long as the numpy array over it"""

    def __init__(self, lib, nbytes):
        self.lib, self.ptr = lib, lib.latok_host_alloc(max(int(nbytes), 1))
        if not self.ptr:
            raise MemoryError(_lib.last_error())

    def __del__(self):
        try:
            self.lib.latok_host_free(self.ptr)
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """np.empty in pinned (page-locked) host memory (latok_host_alloc): host-pointer batches held in such arrays cross the
    bus at full speed and asynchronously, which is what lets the chunked pipeline of the large-batch calls overlap the
    upload of one chunk with the download of another.  The memory is freed when the array (and its views) are gone."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    owner = _Pinned(_lib.ensure_init(), n * dt.itemsize)
    buf = (C.c_char * max(n * dt.itemsize, 1)).from_address(owner.ptr)
    buf._latok_owner = owner
    a = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    return a


def _out_dtype(dtype):
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.int64), np.dtype(np.int32)):
        raise ValueError("dtype must be int64 or int32")
    return dt, (_lib.OUT_INT32 if dt == np.dtype(np.int32) else 0)


def _compact(fn, lead, n_str, total, width, dtype, feats=False, pinned=False):
    """Shared body of the compaction wrappers: fn(*lead, n_str, total, counts, items[, features], cap, &n, flags, stream).
    Returns (counts[n_str], items[n] or items[n, width][, features int8[n, 25]]); counts / items in `dtype` (int64, or
    int32 = LATOK_OUT_INT32: half the bytes written on the device and moved over the bus).  pinned: the result arrays
    live in pinned host memory and are returned as views (no copy)."""
    dt, flags = _out_dtype(dtype)
    alloc = pinned_empty if pinned else np.empty
    counts = alloc(n_str, dt)
    cap = max(total, 1)                                  # a string has at most len items
    items = alloc((cap, width) if width > 1 else cap, dt)
    feat = alloc((cap, _lib.FEATURE_COUNT), np.int8) if feats else None
    n = C.c_int64(0)
    args = list(lead) + [n_str, total, _ptr(counts), _ptr(items)] + ([_ptr(feat)] if feats else []) + [cap, C.byref(n), flags, None]
    _lib.check(fn(*args))
    keep = (lambda a: a) if pinned else (lambda a: a.copy())
    if feats:
        return counts, keep(items[:n.value]), keep(feat[:n.value])
    return counts, keep(items[:n.value])


def split_mask_batch(cps, row_off) -> np.ndarray:
    """Boundary bitmask uint64[ceil(total/64)]: bit i = packed char i starts a token."""
    cps, row_off = _csr(cps, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    bits = np.zeros((total + 63) // 64, np.uint64)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_split_mask_batch(_ptr(cps), _ptr(row_off), n_str, total, _ptr(bits), 0, None))
    return bits


def split_values_batch(cps, row_off) -> np.ndarray:
    """The reference's split values (0..5) for every packed char, uint8[total]."""
    cps, row_off = _csr(cps, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    vals = np.zeros(total, np.uint8)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_split_values_batch(_ptr(cps), _ptr(row_off), n_str, total, _ptr(vals), 0, None))
    return vals


def split_offsets_csr(cps, row_off, dtype=np.int64):
    """(counts[n], offsets[sum(counts)]): per-string boundary offsets, concatenated (dtype int64 or int32)."""
    cps, row_off = _csr(cps, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_split_offsets_batch, [_ptr(cps), _ptr(row_off)], n_str, total, 1, dtype)


# host batches beyond the library's small-batch path (api.cpp: kSmallChars / kSmallStrings, served from pinned memory
# in UTF-32) are shipped as the narrowest PEP 393 kind: 1 or 2 bytes per char over the bus instead of 4
_SMALL_CHARS, _SMALL_STRINGS = 262144, 16384     # api.cpp: kSmallChars / kSmallStrings (pinned zero-copy path)
_ONE_MAX = 16384                                   # split_offsets_one: the per-thread output array


_ROW1 = None


def split_offsets_one(text: str) -> np.ndarray:
    """np.nonzero(split mask)[0] of ONE non-empty string with as little Python around the C call as possible (the drop-in
    tokenize(text) surface): a string of at most 4096 chars is one single-wave launch in the library, which polls the
    kernel's completion word; what is left here is the UTF-32 encode (the bytes object goes to the C call as it is) and
    a copy of the offsets out of a per-thread output array."""
    global _ROW1
    n = len(text)
    if n > _ONE_MAX:
        return split_offsets_batch([text])[0]
    lib = _lib.ensure_init()
    if _ROW1 is None:
        _ROW1 = threading.local()
    st = getattr(_ROW1, "st", None)
    if st is None:
        row, count, offs, n_out = np.zeros(2, np.int64), np.zeros(1, np.int32), np.empty(_ONE_MAX, np.int32), C.c_int64(0)
        st = _ROW1.st = (row, count, offs, n_out, row.ctypes.data, count.ctypes.data, offs.ctypes.data, C.byref(n_out))
    row, _, offs, n_out, p_row, p_count, p_offs, p_n = st
    row[1] = n
    rc = lib.latok_split_offsets_batch(text.encode("utf-32-le", "surrogatepass"), p_row, 1, n, p_count, p_offs, n, p_n,
                                       _lib.OUT_INT32, None)
    if rc:
        _lib.check(rc)
    return offs[:n_out.value].copy()


def featurize_one(text: str):
    """list(featurize(text)) of the reference for ONE non-empty string of at most 4096 chars: two small launches in the
    library (boundaries + kept tokens, then the sums), per-thread output arrays, one LaToken per kept token."""
    from .core.latok_utils import LaToken
    global _FEAT1
    n = len(text)
    if n > 4096:
        return featurize_batch([text])[0]
    lib = _lib.ensure_init()
    if _FEAT1 is None:
        _FEAT1 = threading.local()
    st = getattr(_FEAT1, "st", None)
    if st is None:
        row, count, spans, n_out = np.zeros(2, np.int64), np.zeros(1, np.int32), np.empty((4096, 4), np.int32), C.c_int64(0)
        feats = np.empty((4096, 25), np.int8)
        st = _FEAT1.st = (row, count, spans, feats, n_out, row.ctypes.data, count.ctypes.data, spans.ctypes.data,
                          feats.ctypes.data, C.byref(n_out))
    row, _, spans, feats, n_out, p_row, p_count, p_spans, p_feats, p_n = st
    row[1] = n
    rc = lib.latok_token_features_batch(text.encode("utf-32-le", "surrogatepass"), p_row, 1, n, p_count, p_spans, p_feats, n,
                                        p_n, _lib.OUT_INT32, None)
    if rc:
        _lib.check(rc)
    k = n_out.value
    rows = feats[:k].copy()            # the tokens' vectors are views of one fresh array, not of the per-thread buffer
    return [LaToken(text[c:d], a, b, rows[j]) for j, (a, b, c, d) in enumerate(spans[:k].tolist())]


_FEAT1 = None


def _record_dtype(row_off):
    """int32 records (LATOK_OUT_INT32: half the device writes and bus traffic) unless a string has 2^31 chars or more"""
    return np.int32 if row_off.size < 2 or int(np.diff(row_off).max()) <= 0x7FFFFFFF else np.int64


def _narrow_pays(texts):
    return len(texts) > _SMALL_STRINGS or sum(map(len, texts)) > _SMALL_CHARS


def split_offsets_batch(texts, devices=None):
    """list[str] -> list of int64 arrays = np.nonzero(split mask)[0] of every string ('' -> empty array).
    devices: a multi.DevicePool or a list of device ids -> the strings are sharded over them (latok_amd.multi)."""
    if len(texts) == 0:
        return []
    if devices is not None:
        from . import multi
        return multi.split_offsets_batch(texts, devices)
    if _narrow_pays(texts):
        counts, offsets = split_offsets_kind_csr(*pack_kind(texts))
    else:
        counts, offsets = split_offsets_csr(*pack(texts))
    return np.split(offsets, np.cumsum(counts)[:-1])


def token_spans_csr(cps, row_off, dtype=np.int64):
    """(counts[n], spans[n_tokens, 2]): [start, end) of every token of every string, already stripped and with
    whitespace-only tokens dropped -- everything reference tokenize() does after np.nonzero, on the device."""
    cps, row_off = _csr(cps, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_spans_batch, [_ptr(cps), _ptr(row_off)], n_str, total, 2, dtype)


def token_features_csr(cps, row_off, dtype=np.int64):
    """(counts[n], spans[n_tokens, 4] = {raw_start, raw_end, strip_start, strip_end}, features int8[n_tokens, 25]):
    reference featurize() for a whole batch, without the n x 25 matrix."""
    cps, row_off = _csr(cps, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_features_batch, [_ptr(cps), _ptr(row_off)], n_str, total, 4, dtype, feats=True)


def featurize_batch(texts, devices=None):
    """list[str] -> list[list[LaToken]], each as list(featurize(text)) of the reference.
    devices: a multi.DevicePool or a list of device ids -> the strings are sharded over them."""
    from .core.latok_utils import LaToken
    if len(texts) == 0:
        return []
    if devices is not None:
        from . import multi
        return multi.featurize_batch(texts, devices)
    if _narrow_pays(texts):
        units, row_off = pack_kind(texts)
        counts, spans, feats = token_features_kind_csr(units, row_off, dtype=_record_dtype(row_off))
    else:
        cps, row_off = pack(texts)
        counts, spans, feats = token_features_csr(cps, row_off, dtype=_record_dtype(row_off))
    out, k = [], 0
    for text, n in zip(texts, counts.tolist()):
        out.append([LaToken(text[c:d], a, b, feats[k + j]) for j, (a, b, c, d) in enumerate(spans[k:k + n].tolist())])
        k += n
    return out


# ---- UTF-8 ingest -------------------------------------------------------------------------------------------------------
def pack_utf8(blobs):
    """list[bytes] (each valid UTF-8) -> (utf8 uint8[total_bytes], byte_off int64[n+1])."""
    lens = np.fromiter((len(b) for b in blobs), dtype=np.int64, count=len(blobs))
    byte_off = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum(lens, out=byte_off[1:])
    return np.frombuffer(b"".join(blobs), dtype=np.uint8), byte_off


def _csr_u8(utf8, byte_off):
    utf8 = np.ascontiguousarray(utf8, dtype=np.uint8)
    byte_off = np.ascontiguousarray(byte_off, dtype=np.int64)
    if byte_off.ndim != 1 or byte_off.size < 1 or (byte_off.size > 1 and utf8.size < int(byte_off[-1])):
        raise ValueError("byte_off must be n_str + 1 offsets into utf8")
    return utf8, byte_off


def utf8_decode_csr(utf8, byte_off):
    """Device decode of a UTF-8 CSR batch -> (cps uint32[total_cps], cp_row_off int64[n+1])."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    cps = np.empty(max(total, 1), np.uint32)
    row = np.zeros(n_str + 1, np.int64)
    n = C.c_int64(0)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_utf8_decode_batch(_ptr(utf8), _ptr(byte_off), n_str, total, _ptr(cps), cps.size, _ptr(row),
                                           C.byref(n), 0, None))
    return cps[:n.value].copy(), row


def split_mask_utf8_csr(utf8, byte_off):
    """(bits uint64[ceil(total_cps/64)], cp_row_off int64[n+1]): boundary bitmask over the decoded code points."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    bits = np.zeros((total + 63) // 64, np.uint64)
    row = np.zeros(n_str + 1, np.int64)
    n = C.c_int64(0)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_split_mask_utf8_batch(_ptr(utf8), _ptr(byte_off), n_str, total, _ptr(bits), bits.size, _ptr(row),
                                               C.byref(n), 0, None))
    return bits[:(n.value + 63) // 64], row


def split_offsets_utf8_csr(utf8, byte_off, dtype=np.int64):
    """(counts, offsets) like split_offsets_csr, input handed over as UTF-8 (1 byte per ASCII char over PCIe).
    Offsets are code-point indices, as the reference reports them for the decoded str."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_split_offsets_utf8_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 1, dtype)


def token_spans_utf8_csr(utf8, byte_off, dtype=np.int64):
    """(counts, spans[n_tokens, 2]) like token_spans_csr for a UTF-8 CSR batch; spans are code-point indices."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_spans_utf8_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 2, dtype)


def token_features_utf8_csr(utf8, byte_off, dtype=np.int64):
    """(counts, spans[n_tokens, 4], features int8[n_tokens, 25]) like token_features_csr for a UTF-8 CSR batch: spans are
    code-point indices, exactly what token_features_csr gives for the decoded text (no UTF-32 copy is made for large batches)."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_features_utf8_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 4, dtype, feats=True)


def featurize_utf8_batch(blobs):
    """list[bytes] (each valid UTF-8) -> list[list[LaToken]], token for token what featurize_batch gives for the decoded
    strings: start_idx / end_idx in code points, text = the decoded string sliced at the stripped span."""
    from .core.latok_utils import LaToken
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, spans, feats = token_features_utf8_csr(utf8, byte_off, dtype=_record_dtype(byte_off))
    out, k = [], 0
    for blob, n in zip(blobs, counts.tolist()):
        text = blob.decode("utf-8", "surrogatepass") if n else ""
        out.append([LaToken(text[c:d], a, b, feats[k + j]) for j, (a, b, c, d) in enumerate(spans[k:k + n].tolist())])
        k += n
    return out


# byte-space forms: the tile kernel reads the UTF-8 bytes itself; every position is a BYTE position in `utf8`
def split_mask_utf8_bytes_csr(utf8, byte_off) -> np.ndarray:
    """uint64 bitmask over the BYTES of the batch: bit i set = byte i is the lead byte of a boundary char."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    bits = np.zeros((total + 63) // 64, np.uint64)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_split_mask_utf8_bytes_batch(_ptr(utf8), _ptr(byte_off), n_str, total, _ptr(bits), 0, None))
    return bits


def split_offsets_utf8_bytes_csr(utf8, byte_off, dtype=np.int64):
    """(counts, offsets): boundary BYTE offsets relative to each string's first byte."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_split_offsets_utf8_bytes_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 1, dtype)


def token_spans_utf8_bytes_csr(utf8, byte_off, dtype=np.int64):
    """(counts, spans[n_tokens, 2]): [start, end) BYTE ranges of the stripped, non-empty tokens of each string."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_spans_utf8_bytes_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 2, dtype)


def token_features_utf8_bytes_csr(utf8, byte_off, dtype=np.int64):
    """(counts, spans4[n_tokens, 4], features int8[n_tokens, 25]): featurize in byte space.  spans4 = {raw start, raw end,
    stripped start, stripped end} as BYTE positions relative to each string's first byte; the feature sums count chars, not
    bytes (they are what token_features_utf8_csr gives for the same token).  Malformed UTF-8 (a continuation byte without a
    lead byte) is refused with ValueError."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    _out_dtype(dtype)   # (a bad argument is a ValueError before any device is asked for)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    return _compact(_lib.ensure_init().latok_token_features_utf8_bytes_batch, [_ptr(utf8), _ptr(byte_off)], n_str, total, 4, dtype,
                    feats=True)


def featurize_utf8_bytes_batch(blobs):
    """list[bytes] (each valid UTF-8) -> list[list[LaToken]] without transcoding anything: text = blob[strip_start:strip_end]
    (bytes), start_idx / end_idx = the raw BYTE range of the token in its blob, features = the reference's 25 sums."""
    from .core.latok_utils import LaToken
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, spans, feats = token_features_utf8_bytes_csr(utf8, byte_off, dtype=_record_dtype(byte_off))
    out, k = [], 0
    for blob, n in zip(blobs, counts.tolist()):
        out.append([LaToken(blob[c:d], a, b, feats[k + j]) for j, (a, b, c, d) in enumerate(spans[k:k + n].tolist())])
        k += n
    return out


def tokenize_utf8_batch(blobs):
    """list[bytes] (UTF-8) -> list[list[bytes]]: the reference's tokens of every string, as UTF-8 slices of the input
    (byte-space path: nothing is transcoded on the host or on the device)."""
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, spans = token_spans_utf8_bytes_csr(utf8, byte_off, dtype=_record_dtype(byte_off))
    out, k = [], 0
    for blob, n in zip(blobs, counts.tolist()):
        out.append([blob[a:b] for a, b in spans[k:k + n].tolist()])
        k += n
    return out


# pre-tokens: the byte ranges a model's pre-tokenizer cuts a string into (GPT-2's pattern on the device; "latok": the tokens above)
_PRETOKENIZERS = {"latok": _lib.PRETOK_LATOK, "gpt2": _lib.PRETOK_GPT2, "cl100k": _lib.PRETOK_CL100K, "spm": _lib.PRETOK_SPM}


def _pretok_code(pretokenizer) -> int:
    """the LATOK_PRETOK_* value of a name; anything else is a ValueError (raised before any device is asked for)"""
    if not isinstance(pretokenizer, str) or pretokenizer not in _PRETOKENIZERS:
        raise ValueError("pretokenizer must be one of %s" % ", ".join(repr(k) for k in _PRETOKENIZERS))
    return _PRETOKENIZERS[pretokenizer]


def pretokens_utf8_csr(utf8, byte_off, pretokenizer="gpt2", dtype=np.int64):
    """(counts, spans[n, 2]): the [start, end) BYTE ranges of every string's pre-tokens (``latok_pretokens_utf8_bytes_batch``).
    ``"gpt2"``: GPT-2's pattern -- every byte of a string lies in exactly one pre-token, whitespace included; ``"cl100k"``: the
    cl100k_base / Llama 3 pattern, likewise; ``"spm"``: SentencePiece's segments -- a lead run of spaces and U+2581, then what follows up
    to the next space, nothing dropped; ``"latok"``: exactly what token_spans_utf8_bytes_csr returns."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    code = _pretok_code(pretokenizer)
    _out_dtype(dtype)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    lib = _lib.ensure_init()

    def fn(u8, off, n, t, *rest):
        return lib.latok_pretokens_utf8_bytes_batch(u8, off, n, t, code, *rest)

    return _compact(fn, [_ptr(utf8), _ptr(byte_off)], n_str, total, 2, dtype)


def pretokenize_utf8_batch(blobs, pretokenizer="gpt2"):
    """list[bytes] (UTF-8) -> list[list[bytes]]: every string's pre-tokens as slices of the input; with ``"gpt2"``, ``"cl100k"`` and ``"spm"`` they join
    back to the string byte for byte."""
    _pretok_code(pretokenizer)
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, spans = pretokens_utf8_csr(utf8, byte_off, pretokenizer, _record_dtype(byte_off))
    out, k = [], 0
    for blob, n in zip(blobs, counts.tolist()):
        out.append([blob[a:b] for a, b in spans[k:k + n].tolist()])
        k += n
    return out


def pretokenize_batch(texts, pretokenizer="gpt2"):
    """list[str] -> list[list[str]]: pretokenize_utf8_batch of the strings' UTF-8 ("surrogatepass"), decoded again"""
    rows = pretokenize_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], pretokenizer)
    return [[p.decode("utf-8", "surrogatepass") for p in row] for row in rows]


# joined token text: the tokens themselves, each string's joined by one separator (what a pre-tokenized corpus holds)
def _sep_byte(sep) -> int:
    """the separator as one byte value; anything else is a ValueError (raised before any device is asked for)"""
    if isinstance(sep, (bytes, bytearray)) and len(sep) == 1:
        return sep[0]
    if isinstance(sep, (int, np.integer)) and not isinstance(sep, bool) and 0 <= int(sep) <= 255:
        return int(sep)
    raise ValueError("sep must be one byte (bytes of length 1, or an int 0..255)")


def _join_csr(utf8, byte_off, sep, dtype, want_counts):
    utf8, byte_off = _csr_u8(utf8, byte_off)
    sep = _sep_byte(sep)
    dt, flags = _out_dtype(dtype)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    lib = _lib.ensure_init()
    cap = max(2 * total, 1)                              # a kept token has >= 1 byte and brings <= 1 separator
    out = np.empty(cap, np.uint8)
    out_off = np.zeros(n_str + 1, np.int64)
    counts = np.zeros(n_str, dt) if want_counts else None
    n = C.c_int64(0)
    _lib.check(lib.latok_join_tokens_utf8_bytes_batch(_ptr(utf8), _ptr(byte_off), n_str, total, sep, _ptr(out), cap, _ptr(out_off),
                                                      _ptr(counts) if want_counts else None, C.byref(n), flags, None))
    return out[:n.value], out_off, counts


def join_tokens_utf8_csr(utf8, byte_off, sep=b" ", dtype=np.int64):
    """(out_bytes uint8[], out_off int64[n+1], counts): every string's stripped, non-empty tokens -- the byte ranges
    token_spans_utf8_bytes_csr reports -- joined by the one-byte ``sep``, all rows back to back: row s =
    out_bytes[out_off[s]:out_off[s+1]] = sep.join(tokens of string s); counts[s] = its number of tokens (``dtype``; out_off is
    always int64).  Cut, joined and written on the device (``latok_join_tokens_utf8_bytes_batch``)."""
    out, out_off, counts = _join_csr(utf8, byte_off, sep, dtype, True)
    return out.copy(), out_off, counts


def join_tokens_utf8_batch(blobs, sep=b" "):
    """list[bytes] (UTF-8) -> list[bytes]: ``sep.join(tokens)`` of every string -- the rows ``[sep.join(t) for t in
    tokenize_utf8_batch(blobs)]`` gives, without a token-by-token loop on the host ('' and whitespace-only -> b'')."""
    sep_b = _sep_byte(sep)
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    out, out_off, _ = _join_csr(utf8, byte_off, sep_b, np.int64, False)
    buf, o = out.tobytes(), out_off.tolist()
    return [buf[a:b] for a, b in zip(o[:-1], o[1:])]


def join_tokens_batch(texts, sep=" "):
    """list[str] -> list[str]: ``sep.join(tokenize(text))`` of every string ('' -> ''); ``sep`` is one ASCII character.  The
    strings go through UTF-8 ("surrogatepass") and the byte-space call; rows are decoded one by one."""
    if not isinstance(sep, str) or len(sep) != 1 or ord(sep) > 0x7F:
        raise ValueError("sep must be one ASCII character")
    rows = join_tokens_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], sep.encode("ascii"))
    return [r.decode("utf-8", "surrogatepass") for r in rows]


# case folding and accent stripping: UTF-8 in, folded UTF-8 out -- what an uncased vocabulary or a lower-casing vectorizer needs in
# front of the token calls (the definition: include/latok_hip.h, latok_fold_utf8_bytes_batch)
FOLD_LOWER, FOLD_STRIP_MARKS, FOLD_CLEAN, FOLD_CJK_SPACE = _lib.FOLD_LOWER, _lib.FOLD_STRIP_MARKS, _lib.FOLD_CLEAN, _lib.FOLD_CJK_SPACE
FOLD_UNCASED = FOLD_LOWER | FOLD_STRIP_MARKS


def _fold_bits(fold) -> int:
    """the fold flags as an int 0 .. 15; anything else is a ValueError (raised before any device is asked for)"""
    if isinstance(fold, (int, np.integer)) and not isinstance(fold, bool) and 0 <= int(fold) <= 15:
        return int(fold)
    raise ValueError("fold must be a combination of the FOLD_* flags (0 .. 15)")


def _fold_csr(utf8, byte_off, fold):
    utf8, byte_off = _csr_u8(utf8, byte_off)
    fold = _fold_bits(fold)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    lib = _lib.ensure_init()
    cap = max(3 * total, 1)                              # an image has at most three times the bytes of its sequence
    out = np.empty(cap, np.uint8)
    out_off = np.zeros(n_str + 1, np.int64)
    n = C.c_int64(0)
    _lib.check(lib.latok_fold_utf8_bytes_batch(_ptr(utf8), _ptr(byte_off), n_str, total, fold, _ptr(out), cap, _ptr(out_off), C.byref(n), 0, None))
    return out[:n.value], out_off


def fold_utf8_csr(utf8, byte_off, fold=FOLD_UNCASED):
    """(out_bytes uint8[], out_off int64[n + 1]): every string folded -- lower-cased (``FOLD_LOWER``), canonically decomposed with
    the nonspacing marks dropped (``FOLD_STRIP_MARKS``), control characters dropped and whitespace turned into U+0020
    (``FOLD_CLEAN``), CJK ideographs set between spaces (``FOLD_CJK_SPACE``); row s = out_bytes[out_off[s]:out_off[s+1]].  Malformed
    bytes and characters that are their own image are copied verbatim.  Folded on the device (``latok_fold_utf8_bytes_batch``)."""
    out, out_off = _fold_csr(utf8, byte_off, fold)
    return out.copy(), out_off


def fold_utf8_batch(blobs, fold=FOLD_UNCASED):
    """list[bytes] (UTF-8) -> list[bytes]: every string folded (fold_utf8_csr) -- with ``FOLD_UNCASED``, for text without a capital
    sigma, ``"".join(c for c in unicodedata.normalize("NFD", t.lower()) if unicodedata.category(c) != "Mn")``."""
    fold = _fold_bits(fold)
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    out, out_off = _fold_csr(utf8, byte_off, fold)
    buf, o = out.tobytes(), out_off.tolist()
    return [buf[a:b] for a, b in zip(o[:-1], o[1:])]


def fold_batch(texts, fold=FOLD_UNCASED):
    """list[str] -> list[str]: fold_utf8_batch of the strings' UTF-8 ("surrogatepass"), decoded row by row."""
    rows = fold_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], fold)
    return [r.decode("utf-8", "surrogatepass") for r in rows]


class _HostBatch:
    """A host batch as a sized call takes it: ``lib``, ``u8`` / ``off`` / ``n_str`` / ``total`` and the call's base ``flags``; the
    call's outputs come from ``out`` (``zero``: the per-string arrays, which start at 0 on the host) and reach the caller through
    ``fetch``.  Here they are plain numpy arrays that the library fills itself: nothing is allocated on the device and nothing
    copied beyond what the library call does."""

    flags = 0
    lib = property(lambda self: _lib.ensure_init())   # (asked for by the call that needs it; Idf.update_utf8 calls through its own)

    def __init__(self, utf8, byte_off):
        self._arrays = utf8, byte_off = _csr_u8(utf8, byte_off)
        self.n_str = byte_off.size - 1
        self.total = int(byte_off[-1]) if self.n_str > 0 else 0
        self.u8, self.off = _ptr(utf8), _ptr(byte_off)

    def out(self, shape, dtype, zero=False):
        return (np.zeros if zero else np.empty)(shape, dtype)

    def fetch(self, buf, n=None):
        """the output itself, or a copy of its first ``n`` rows (never a view of an oversized buffer)"""
        return buf if n is None else buf[:n].copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


class _DeviceFolded:
    """The interface of _HostBatch over a host batch folded into device memory: the batch is uploaded once and folded there
    (``latok_fold_utf8_bytes_batch`` with device pointers); the call runs with ``LATOK_DEVICE_PTRS`` on device buffers, which
    ``fetch`` copies to the host.  No folded byte visits the host.  Everything is freed on leaving the ``with`` block."""

    flags = _lib.DEVICE_PTRS

    def __init__(self, utf8, byte_off, fold):
        utf8, byte_off = _csr_u8(utf8, byte_off)
        self.lib, self._bufs, self._outs = _lib.ensure_init(), [], {}
        self.n_str = byte_off.size - 1
        total = int(byte_off[-1]) if self.n_str > 0 else 0
        try:
            src, src_off = self.alloc(total), self.alloc(byte_off.nbytes)
            self.u8, self.off = self.alloc(3 * total), self.alloc(byte_off.nbytes)
            if total > 0:
                _lib.check(self.lib.latok_memcpy_h2d(src, _ptr(utf8), total))
            _lib.check(self.lib.latok_memcpy_h2d(src_off, _ptr(byte_off), byte_off.nbytes))
            n = C.c_int64(0)
            _lib.check(self.lib.latok_fold_utf8_bytes_batch(src, src_off, self.n_str, total, fold, self.u8, max(3 * total, 1), self.off, C.byref(n),
                                                            _lib.DEVICE_PTRS, None))
            self.total = n.value
        except Exception:
            self.close()
            raise

    def alloc(self, nbytes):
        p = self.lib.latok_dev_alloc(int(nbytes) + 64)
        if not p:
            raise MemoryError(_lib.last_error())
        self._bufs.append(p)
        return p

    def out(self, shape, dtype, zero=False):
        shape = shape if isinstance(shape, tuple) else (int(shape),)
        p = self.alloc(int(np.prod(shape)) * np.dtype(dtype).itemsize)
        self._outs[p] = shape, dtype
        return p

    def fetch(self, buf, n=None):
        shape, dtype = self._outs[buf]
        out = np.empty(shape if n is None else (n,) + shape[1:], dtype)
        if out.nbytes > 0:
            _lib.check(self.lib.latok_memcpy_d2h(_ptr(out), buf, out.nbytes))
        return out

    def close(self):
        bufs, self._bufs = self._bufs, []
        for p in bufs:
            self.lib.latok_dev_free(p)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _batch_on(utf8, byte_off, fold):
    """the batch of a sized call: the host arrays as they are, or (``fold``, FOLD_* flags) their folded image in device memory"""
    return _DeviceFolded(utf8, byte_off, fold) if fold else _HostBatch(utf8, byte_off)


def _arg(buf):
    """an output of ``out`` (or None) as a ctypes argument"""
    return _ptr(buf) if isinstance(buf, np.ndarray) else buf


def _size_then_fill(call, n, alloc):
    """The capacity protocol of the sized calls.  ``call()`` is the size query (no buffer, cap = 0): it reports its need into ``n``, a
    c_int64, and may refuse the capacity.  ``alloc(need)`` then makes the payload buffers -- outputs of the batch's ``out``, or
    None -- and ``call(*buffers, need)`` fills them, unless nothing is needed.  Returns (need, buffers)."""
    rc = call()
    if rc != _lib.OK and not (rc == _lib.ERR_INVALID and n.value > 0):
        _lib.check(rc)
    need = n.value
    bufs = alloc(need)
    if need > 0:
        _lib.check(call(*[_arg(b) for b in bufs], need))
    return need, bufs


class _DeviceObject:
    """What Vocab, WordPiece, BPE, Unigram, Detokenizer, Idf and TokenCounter share: ``handle`` (None once closed) of an object that ``_lib`` made and its call
    named ``_destroy`` frees -- by ``close()``, on leaving a ``with`` block, or with the object.  ``_closed``: what ``_open()`` says."""

    handle = _destroy = _closed = None

    def _open(self):
        if not self.handle:
            raise ValueError(self._closed)
        return self.handle

    def close(self):
        if self.handle:
            h, self.handle = self.handle, None
            _lib.check(getattr(self._lib, self._destroy)(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _handle_of(cls, obj, name, or_none=False):
    """the handle of an open ``cls`` passed as argument ``name``; None for None where the call takes that"""
    if obj is None and or_none:
        return None
    if not isinstance(obj, cls) or not obj.handle:
        raise ValueError("%s must be an open latok_amd.batch.%s%s" % (name, cls.__name__, " or None" if or_none else ""))
    return obj.handle


def _int32_each(values, n, name, per):
    """``values`` as int32[n]; anything but one integer per ``per`` that fits int32 is a ValueError"""
    raw = np.asarray(values)
    if raw.shape != (n,) or (raw.size and raw.dtype.kind not in "iu"):
        raise ValueError("%s must be one integer per %s" % (name, per))
    if raw.size and (raw.min() < -0x80000000 or raw.max() > 0x7FFFFFFF):
        raise ValueError("%s must fit int32" % name)
    return np.ascontiguousarray(raw, np.int32)


def _pack_words(words, ids):
    """the words of a Vocab or WordPiece (``bytes``, or ``str`` as UTF-8 with surrogatepass) and their optional ids ->
    (data uint8[total], off int64[n + 1], ids int32[n] or None)"""
    blobs = [w.encode("utf-8", "surrogatepass") if isinstance(w, str) else bytes(w) for w in words]
    data, off = pack_utf8(blobs)
    return data, off, None if ids is None else _int32_each(ids, len(blobs), "ids", "word")


# token hashes: one 32-bit id per token (MurmurHash3 x86_32 of its UTF-8 bytes) -- what hashing vectorizers and hashed tables take
def murmur3_32(data: bytes, seed=0) -> int:
    """MurmurHash3 x86_32 of ``data`` (bytes) with a 32-bit ``seed``, as an unsigned int: the word the device gives for a token with
    these bytes (``token_hashes_*``), computed on the host -- for building id tables from a vocabulary.  scikit-learn's
    ``murmurhash3_32(data, seed, positive=True)`` is the same number."""
    seed = _seed32(seed)
    data = bytes(data)
    m = 0xFFFFFFFF
    h, n = seed, len(data)
    for i in range(0, n & ~3, 4):
        k = int.from_bytes(data[i:i + 4], "little") * 0xcc9e2d51 & m
        k = ((k << 15) | (k >> 17)) * 0x1b873593 & m
        h ^= k
        h = (((h << 13) & m | (h >> 19)) * 5 + 0xe6546b64) & m
    if n & 3:
        k = int.from_bytes(data[n & ~3:], "little") * 0xcc9e2d51 & m
        k = (((k << 15) & m) | (k >> 17)) * 0x1b873593 & m
        h ^= k
    h ^= n & m
    h = (h ^ (h >> 16)) * 0x85ebca6b & m
    h = (h ^ (h >> 13)) * 0xc2b2ae35 & m
    return h ^ (h >> 16)


def _seed32(seed) -> int:
    """the seed as an int 0 .. 2**32 - 1; anything else is a ValueError (raised before any device is asked for)"""
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool) and 0 <= int(seed) <= 0xFFFFFFFF:
        return int(seed)
    raise ValueError("seed must be an int in 0 .. 2**32 - 1")


def _hashes_csr(utf8, byte_off, seed, dtype, want_spans):
    utf8, byte_off = _csr_u8(utf8, byte_off)
    seed = _seed32(seed)
    dt, flags = _out_dtype(dtype)
    n_str = byte_off.size - 1
    total = int(byte_off[-1]) if n_str > 0 else 0
    lib = _lib.ensure_init()
    cap = max(total, 1)                                  # a token has at least one byte
    counts = np.zeros(n_str, dt)
    hashes = np.empty(cap, np.uint32)
    spans = np.empty((cap, 2), dt) if want_spans else None
    n = C.c_int64(0)
    _lib.check(lib.latok_token_hashes_utf8_bytes_batch(_ptr(utf8), _ptr(byte_off), n_str, total, seed, _ptr(counts),
                                                       _ptr(spans) if want_spans else None, _ptr(hashes), cap, C.byref(n), flags, None))
    return counts, hashes[:n.value].copy(), (spans[:n.value].copy() if want_spans else None)


def token_hashes_utf8_csr(utf8, byte_off, seed=0, dtype=np.int64, spans=False):
    """(counts, hashes uint32[n_tokens][, spans[n_tokens, 2]]): MurmurHash3 x86_32 (``seed``) of the UTF-8 bytes of every stripped,
    non-empty token -- the byte ranges token_spans_utf8_bytes_csr reports, in its order: hashes[k] belongs to spans[k].  counts
    (and spans, with ``spans=True``) in ``dtype``.  Cut and hashed on the device (``latok_token_hashes_utf8_bytes_batch``); the
    host sees no token text.  ``murmur3_32(token_bytes, seed)`` is the same word."""
    counts, hashes, sp = _hashes_csr(utf8, byte_off, seed, dtype, spans)
    return (counts, hashes, sp) if spans else (counts, hashes)


def token_hashes_utf8_batch(blobs, seed=0):
    """list[bytes] (UTF-8) -> list of uint32 arrays: the hashes of every string's tokens ('' and whitespace-only -> empty)."""
    seed = _seed32(seed)
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, hashes, _ = _hashes_csr(utf8, byte_off, seed, np.int64, False)
    return np.split(hashes, np.cumsum(counts)[:-1])


def token_hashes_batch(texts, seed=0):
    """list[str] -> list of uint32 arrays: ``[murmur3_32(t.encode("utf-8"), seed) for t in tokenize(text)]`` of every string.  The
    strings go through UTF-8 ("surrogatepass") on the host and the byte-space call."""
    seed = _seed32(seed)
    return token_hashes_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], seed)


# token ids: every token's id in a vocabulary, looked up on the device -- exact (the bytes decide, the hash only finds the slot)
def _unk32(unk_id) -> int:
    """unk_id as an int32; anything else is a ValueError (raised before any device is asked for)"""
    if isinstance(unk_id, (int, np.integer)) and not isinstance(unk_id, bool) and -0x80000000 <= int(unk_id) <= 0x7FFFFFFF:
        return int(unk_id)
    raise ValueError("unk_id must be an int in -2**31 .. 2**31 - 1")


class Vocab(_DeviceObject):
    """A vocabulary on the device of the current context (``latok_vocab_create``): ``words`` is a list of ``bytes`` or ``str``
    (``str`` is encoded as UTF-8 with surrogatepass), ``ids`` an optional int32 per word (default: its index), ``seed`` the 32-bit
    seed of the table's hash.  Of a duplicate word the first wins; the empty word never matches.  Immutable; ``len()`` is the
    number of words given, ``.n_slots`` the size of the table.  Freed by ``close()``, on leaving a ``with`` block, or with the
    object."""

    _destroy, _closed = "latok_vocab_destroy", "vocab must be an open latok_amd.batch.Vocab"

    def __init__(self, words, ids=None, seed=0):
        seed = _seed32(seed)
        data, off, ids = _pack_words(words, ids)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        _lib.check(lib.latok_vocab_create(_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(ids) if ids is not None else None,
                                          seed, C.byref(h)))
        self._lib, self.handle, self.seed, self._n = lib, h, seed, off.size - 1
        n_slots = C.c_int64(0)
        _lib.check(lib.latok_vocab_info(h, None, C.byref(n_slots), None, None))
        self.n_slots = n_slots.value

    def __len__(self):
        return self._n


def _ids_csr(utf8, byte_off, vocab, unk_id, dtype, want_spans, fold=0):
    utf8, byte_off = _csr_u8(utf8, byte_off)
    unk_id = _unk32(unk_id)
    dt, flags = _out_dtype(dtype)
    handle = _handle_of(Vocab, vocab, "vocab")
    with _batch_on(utf8, byte_off, fold) as b:
        cap = max(b.total, 1)                            # a token has at least one byte
        counts, ids, spans = b.out(b.n_str, dt, True), b.out(cap, np.int32), (b.out((cap, 2), dt) if want_spans else None)
        n = C.c_int64(0)
        _lib.check(b.lib.latok_token_ids_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, handle, unk_id, _arg(counts), _arg(spans), _arg(ids), cap,
                                                          C.byref(n), flags | b.flags, None))
        return b.fetch(counts), b.fetch(ids, n.value), (b.fetch(spans, n.value) if want_spans else None)


def token_ids_utf8_csr(utf8, byte_off, vocab, unk_id=-1, dtype=np.int64, spans=False):
    """(counts, ids int32[n_tokens][, spans[n_tokens, 2]]): the id in ``vocab`` of every stripped, non-empty token -- the byte
    ranges token_spans_utf8_bytes_csr reports, in its order: ids[k] belongs to spans[k] --, ``unk_id`` where the vocabulary does
    not hold the token's bytes.  counts (and spans, with ``spans=True``) in ``dtype``.  Cut, hashed and looked up on the device
    (``latok_token_ids_utf8_bytes_batch``); the host sees no token text."""
    counts, ids, sp = _ids_csr(utf8, byte_off, vocab, unk_id, dtype, spans)
    return (counts, ids, sp) if spans else (counts, ids)


def token_ids_utf8_batch(blobs, vocab, unk_id=-1, fold=0):
    """list[bytes] (UTF-8) -> list of int32 arrays: the ids of every string's tokens ('' and whitespace-only -> empty).  ``fold``
    (FOLD_* flags): the batch is folded on the device first (fold_utf8_batch) and the tokens are those of the folded strings."""
    unk_id, fold = _unk32(unk_id), _fold_bits(fold)
    _handle_of(Vocab, vocab, "vocab")
    if len(blobs) == 0:
        return []
    utf8, byte_off = pack_utf8(blobs)
    counts, ids, _ = _ids_csr(utf8, byte_off, vocab, unk_id, np.int64, False, fold)
    return np.split(ids, np.cumsum(counts)[:-1])


def token_ids_batch(texts, vocab, unk_id=-1):
    """list[str] -> list of int32 arrays: ``[d.get(t.encode("utf-8"), unk_id) for t in tokenize(text)]`` of every string, d =
    the vocabulary as a dict.  The strings go through UTF-8 ("surrogatepass") on the host and the byte-space call."""
    unk_id = _unk32(unk_id)
    return token_ids_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], vocab, unk_id)


# term counts: every string's distinct tokens with their counts -- the CSR rows of a document-term matrix, built on the device
def _n_features31(n_features) -> int:
    """n_features as an int 1 .. 2**31 - 1; anything else is a ValueError (raised before any device is asked for)"""
    if isinstance(n_features, (int, np.integer)) and not isinstance(n_features, bool) and 1 <= int(n_features) <= 0x7FFFFFFF:
        return int(n_features)
    raise ValueError("n_features must be an int in 1 .. 2**31 - 1")


NGRAM_MAX = 8   # kNgMax of the library: the highest order of a word n-gram


def _ngram_spec(ngram_range, sep):
    """(min_n, max_n, sep byte) of a call that counts word n-grams, None for ngram_range (1, 1): the plain term counts.  Anything but
    two ints 1 <= min_n <= max_n <= NGRAM_MAX and a one-byte separator is a ValueError (raised before any device is asked for)."""
    sep = _sep_byte(sep)
    ok = isinstance(ngram_range, (tuple, list)) and len(ngram_range) == 2 and all(
        isinstance(n, (int, np.integer)) and not isinstance(n, bool) for n in ngram_range)
    if not ok or not 1 <= int(ngram_range[0]) <= int(ngram_range[1]) <= NGRAM_MAX:
        raise ValueError("ngram_range must be (min_n, max_n) with 1 <= min_n <= max_n <= %d" % NGRAM_MAX)
    min_n, max_n = int(ngram_range[0]), int(ngram_range[1])
    return None if (min_n, max_n) == (1, 1) else (min_n, max_n, sep)


def _analyzer_spec(analyzer, ngram_range, sep, pad):
    """What the term counts count: ``analyzer="word"`` gives _ngram_spec (None: the plain term counts), ``"char_wb"`` gives
    ("char_wb", min_n, max_n, pad byte) -- character n-grams inside every token's padded word, ``ngram_range`` the character range
    ((1, 1) is a real request there) and ``sep`` ignored.  Anything else is a ValueError (raised before any device is asked for)."""
    if isinstance(analyzer, str) and analyzer == "word":
        return _ngram_spec(ngram_range, sep)
    if not (isinstance(analyzer, str) and analyzer == "char_wb"):
        raise ValueError('analyzer must be "word" or "char_wb"')
    if not (isinstance(pad, (bytes, bytearray)) and len(pad) == 1) and not (
            isinstance(pad, (int, np.integer)) and not isinstance(pad, bool) and 0 <= int(pad) <= 255):
        raise ValueError("pad must be one byte (bytes of length 1, or an int 0..255)")
    _ngram_spec(ngram_range, b" ")   # (the range check)
    return "char_wb", int(ngram_range[0]), int(ngram_range[1]), pad[0] if isinstance(pad, (bytes, bytearray)) else int(pad)


def _rows_csr(utf8, byte_off, fold, dtype, hashed, data_dtype, entry):
    """The sized CSR families (term counts, TF-IDF) on either batch: the size query, then the fill -> (indptr, indices, data, oov or
    None).  ``entry(b, indptr, oov, indices, data, cap, nnz, flags)`` is the library call on batch ``b``."""
    dt, flags = _out_dtype(dtype)
    with _batch_on(utf8, byte_off, fold) as b:
        indptr, oov = b.out(b.n_str + 1, dt, True), None if hashed else b.out(b.n_str, dt, True)
        nnz = C.c_int64(0)

        def call(indices=None, data=None, cap=0):
            return entry(b, _arg(indptr), _arg(oov), indices, data, cap, nnz, flags | b.flags)

        _, (indices, data) = _size_then_fill(call, nnz, lambda k: (b.out(k, np.int32), b.out(k, data_dtype)))
        return b.fetch(indptr), b.fetch(indices), b.fetch(data), None if hashed else b.fetch(oov)


def _terms_call(b, ng, hashed, vocab, indptr, oov, indices, data, cap, nnz, flags):
    """one call of the term counts: the n-gram entry points when ``ng`` is set (the character n-gram ones when it is a "char_wb"
    spec), else the existing ones exactly as they were"""
    lib, batch = b.lib, (b.u8, b.off, b.n_str, b.total)
    if ng and ng[0] == "char_wb":
        if hashed:
            seed, n_features, alternate_sign = hashed
            return lib.latok_hashed_chargram_counts_utf8_bytes_batch(*batch, seed, n_features, 1 if alternate_sign else 0, ng[1], ng[2], ng[3],
                                                                     indptr, indices, data, cap, C.byref(nnz), None, flags, None)
        return lib.latok_chargram_counts_utf8_bytes_batch(*batch, vocab, ng[1], ng[2], ng[3], indptr, oov, indices, data, cap, C.byref(nnz), None,
                                                          flags, None)
    if hashed:
        seed, n_features, alternate_sign = hashed
        if ng:
            return lib.latok_hashed_ngram_counts_utf8_bytes_batch(*batch, seed, n_features, 1 if alternate_sign else 0, ng[0], ng[1], ng[2], indptr,
                                                                  indices, data, cap, C.byref(nnz), None, flags, None)
        return lib.latok_hashed_term_counts_utf8_bytes_batch(*batch, seed, n_features, 1 if alternate_sign else 0, indptr, indices, data, cap,
                                                             C.byref(nnz), None, flags, None)
    if ng:
        return lib.latok_ngram_counts_utf8_bytes_batch(*batch, vocab, ng[0], ng[1], ng[2], indptr, oov, indices, data, cap, C.byref(nnz), None, flags,
                                                       None)
    return lib.latok_term_counts_utf8_bytes_batch(*batch, vocab, indptr, oov, indices, data, cap, C.byref(nnz), None, flags, None)


def _terms_csr(utf8, byte_off, vocab, hashed, dtype, ng=None, fold=0):
    """(indptr, indices, data, oov or None) of the batch, or (``fold``) of its folded image"""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    return _rows_csr(utf8, byte_off, fold, dtype, hashed, np.int32, lambda b, *out: _terms_call(b, ng, hashed, vocab, *out))


def term_counts_utf8_csr(utf8, byte_off, vocab, dtype=np.int64, ngram_range=(1, 1), sep=b" ", analyzer="word", pad=b" "):
    """(indptr[n + 1], indices int32[nnz], data int32[nnz], oov[n]): the term counts of every string against ``vocab`` as a
    canonical CSR matrix -- row s holds the distinct vocabulary ids of its tokens (the byte slices token_spans_utf8_bytes_csr
    reports), ascending, each with its count; ``oov[s]`` counts the tokens the vocabulary does not hold.  What
    ``CountVectorizer(vocabulary=...).transform`` returns: ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n_cols))``.
    indptr and oov in ``dtype``.  Cut, looked up, sorted and reduced on the device (``latok_term_counts_utf8_bytes_batch``).
    ``ngram_range=(min_n, max_n)`` (up to (8, 8)) counts word n-grams instead: every run of n neighbouring tokens of a string joined by the one-byte ``sep``, for every n
    in the range, looked up or hashed as one term -- scikit-learn's ``ngram_range`` (``latok_ngram_counts_utf8_bytes_batch`` /
    ``latok_hashed_ngram_counts_utf8_bytes_batch``); (1, 1) takes the plain calls.
    A vocabulary word may hold the separator (``b"new york"``).
    ``analyzer="char_wb"`` counts character n-grams inside tokens instead (scikit-learn's analyzer of that name over
    ``" ".join(tokens)``): every token is padded with the one-byte ``pad`` on both sides, ``ngram_range`` is the range in CHARACTERS
    (a character starts at every byte that is no UTF-8 continuation byte; (1, 1) is a real request), a padded word shorter than n
    counts once, and ``sep`` is ignored (``latok_chargram_counts_utf8_bytes_batch`` / ``latok_hashed_chargram_counts_utf8_bytes_batch``).
    A vocabulary word may hold the pad (``b" th"``).  ``analyzer="word"`` is the default; anything else is a ValueError."""
    return _terms_csr(utf8, byte_off, _handle_of(Vocab, vocab, "vocab"), None, dtype, _analyzer_spec(analyzer, ngram_range, sep, pad))


def term_counts_utf8_batch(blobs, vocab, fold=0, ngram_range=(1, 1), sep=b" ", analyzer="word", pad=b" "):
    """list[bytes] (UTF-8) -> (indptr, indices, data, oov) of term_counts_utf8_csr, int64 ('' and whitespace-only -> empty rows).
    ``fold`` (FOLD_* flags): the batch is folded on the device first (fold_utf8_batch) -- ``CountVectorizer(lowercase=True)`` is
    ``FOLD_LOWER``, ``strip_accents="unicode"`` adds ``FOLD_STRIP_MARKS``.  ``ngram_range``, ``sep``, ``analyzer``, ``pad``: as in
    term_counts_utf8_csr; the grams are those of the folded strings."""
    handle, fold, ng = _handle_of(Vocab, vocab, "vocab"), _fold_bits(fold), _analyzer_spec(analyzer, ngram_range, sep, pad)
    utf8, byte_off = pack_utf8(blobs)
    return _terms_csr(utf8, byte_off, handle, None, np.int64, ng, fold)


def term_counts_batch(texts, vocab, ngram_range=(1, 1), sep=b" ", analyzer="word", pad=b" "):
    """list[str] -> (indptr, indices, data, oov): per string ``Counter(d[t] for t in tokenize(text) if t in d)`` with sorted keys,
    d = the vocabulary as a dict; oov = the tokens not in d.  The strings go through UTF-8 ("surrogatepass") on the host.
    ``ngram_range``, ``sep``, ``analyzer``, ``pad``: as in term_counts_utf8_csr."""
    return term_counts_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], vocab, ngram_range=ngram_range, sep=sep, analyzer=analyzer,
                                  pad=pad)


def hashed_term_counts_utf8_csr(utf8, byte_off, n_features=1 << 20, seed=0, alternate_sign=True, dtype=np.int64, ngram_range=(1, 1), sep=b" ",
                                analyzer="word", pad=b" "):
    """(indptr[n + 1], indices int32[nnz], data int32[nnz]): the hashed term counts of every string as a canonical CSR matrix --
    column = ``abs(h) % n_features``, value = ``+1`` or (``alternate_sign`` and h < 0) ``-1``, h = MurmurHash3 x86_32 of the token's
    bytes with ``seed`` as int32; a row's columns ascend and a sum may be an explicit 0.  What ``HashingVectorizer(norm=None)
    .transform`` returns: ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(n, n_features))``.  indptr in ``dtype``.  Cut,
    hashed, sorted and reduced on the device (``latok_hashed_term_counts_utf8_bytes_batch``).  ``ngram_range``, ``sep``: word n-grams,
    ``analyzer="char_wb"``, ``pad``: character n-grams inside tokens, as in term_counts_utf8_csr."""
    return _terms_csr(utf8, byte_off, None, (_seed32(seed), _n_features31(n_features), bool(alternate_sign)), dtype,
                      _analyzer_spec(analyzer, ngram_range, sep, pad))[:3]


def hashed_term_counts_utf8_batch(blobs, n_features=1 << 20, seed=0, alternate_sign=True, fold=0, ngram_range=(1, 1), sep=b" ", analyzer="word",
                                  pad=b" "):
    """list[bytes] (UTF-8) -> (indptr, indices, data) of hashed_term_counts_utf8_csr, int64.  ``fold`` (FOLD_* flags): the batch is
    folded on the device first (fold_utf8_batch); ``HashingVectorizer`` lower-cases by default: ``FOLD_LOWER``.  ``ngram_range``, ``sep``,
    ``analyzer``, ``pad``: as in hashed_term_counts_utf8_csr; the grams are those of the folded strings."""
    hashed, fold = (_seed32(seed), _n_features31(n_features), bool(alternate_sign)), _fold_bits(fold)
    ng = _analyzer_spec(analyzer, ngram_range, sep, pad)
    utf8, byte_off = pack_utf8(blobs)
    return _terms_csr(utf8, byte_off, None, hashed, np.int64, ng, fold)[:3]


def hashed_term_counts_batch(texts, n_features=1 << 20, seed=0, alternate_sign=True, ngram_range=(1, 1), sep=b" ", analyzer="word", pad=b" "):
    """list[str] -> (indptr, indices, data): hashed_term_counts_utf8_batch of the strings' UTF-8 ("surrogatepass")."""
    return hashed_term_counts_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], n_features, seed, alternate_sign, ngram_range=ngram_range,
                                         sep=sep, analyzer=analyzer, pad=pad)


# TF-IDF: document frequencies over many batches and the float32 weighting of the CSR rows, on the device -- TfidfVectorizer's last step
def _tfidf_opts(smooth_idf, sublinear_tf, norm) -> int:
    """the LATOK_TFIDF_* bits of a call; ``norm`` is "l1", "l2" or None, anything else a ValueError (before any device is asked for)"""
    if norm not in ("l1", "l2", None):
        raise ValueError('norm must be "l1", "l2" or None')
    return ((_lib.TFIDF_SMOOTH_IDF if smooth_idf else 0) | (_lib.TFIDF_SUBLINEAR_TF if sublinear_tf else 0) |
            (_lib.TFIDF_NORM_L1 if norm == "l1" else _lib.TFIDF_NORM_L2 if norm == "l2" else 0))


def _csr_arrays(indptr, indices, data=None):
    """(indptr int32 or int64, indices int32[, data int32], flags): contiguous copies where needed; the width of indptr picks the flag"""
    indptr = np.asarray(indptr)
    if indptr.ndim != 1 or indptr.size < 1 or indptr.dtype.kind not in "iu":
        raise ValueError("indptr must be a 1-d integer array of n_rows + 1 entries")
    indptr = np.ascontiguousarray(indptr, np.int32 if indptr.dtype == np.int32 else np.int64)
    indices = np.ascontiguousarray(indices, np.int32)
    flags = _lib.OUT_INT32 if indptr.dtype == np.int32 else 0
    if data is None:
        return indptr, indices, flags
    data = np.ascontiguousarray(data, np.int32)
    if data.shape != indices.shape or data.ndim != 1:
        raise ValueError("indices and data must be 1-d arrays of one length")
    return indptr, indices, data, flags


class Idf(_DeviceObject):
    """Document frequencies on the device of the current context (``latok_idf_create``): ``df[n_cols]`` -- in how many rows a column
    was stored -- and ``n_docs``, accumulated over any number of batches; ``weights()`` is the idf vector ``ln((n_docs + s) / (df + s)) +
    1`` (s = 1 if smooth), float32, what ``TfidfTransformer.idf_`` holds after ``fit``.  ``df()`` hands a caller what ``min_df`` /
    ``max_df`` pruning needs.  Freed by ``close()``, on leaving a ``with`` block, or with the object."""

    _destroy, _closed = "latok_idf_destroy", "the idf is closed"

    def __init__(self, n_cols):
        if not isinstance(n_cols, (int, np.integer)) or isinstance(n_cols, bool):
            raise ValueError("n_cols must be an int in 1 .. 2**28")
        lib = _lib.ensure_init()
        h = C.c_void_p()
        _lib.check(lib.latok_idf_create(int(n_cols), C.byref(h)))
        self._lib, self.handle, self.n_cols = lib, h, int(n_cols)

    def update_csr(self, indptr, indices):
        """df[c] += 1 for every stored entry of the CSR (explicit zeros count), n_docs += n_rows: ``np.bincount(indices)``"""
        indptr, indices, flags = _csr_arrays(indptr, indices)
        _lib.check(self._lib.latok_idf_update_csr(self._open(), _ptr(indptr), _ptr(indices) if indices.size else None, indptr.size - 1,
                                                  indices.size, flags, None))

    def update_utf8(self, blobs, vocab=None, n_features=None, seed=0, fold=0, ngram_range=(1, 1), sep=b" "):
        """The same update straight from text, list[bytes] (UTF-8): the rows of term_counts_utf8_batch (``vocab``) or of
        hashed_term_counts_utf8_batch (``n_features``, ``seed``) -- exactly one of the two -- are counted on the device and never
        visit the host.  Returns nnz, the entries the batch stored."""
        if (vocab is None) == (n_features is None):
            raise ValueError("exactly one of vocab and n_features must be given")
        handle = None if vocab is None else _handle_of(Vocab, vocab, "vocab")
        n_feat, seed = (0 if n_features is None else _n_features31(n_features)), _seed32(seed)
        fold, ng = _fold_bits(fold), _ngram_spec(ngram_range, sep) or (1, 1, _sep_byte(sep))
        h, nnz = self._open(), C.c_int64(0)
        utf8, byte_off = pack_utf8(blobs)
        with _batch_on(utf8, byte_off, fold) as b:
            _lib.check(self._lib.latok_idf_update_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, handle, seed, n_feat, ng[0], ng[1], ng[2], h,
                                                                   C.byref(nnz), None, b.flags, None))
        return nnz.value

    def update(self, texts, **kw):
        """list[str]: update_utf8 of the strings' UTF-8 ("surrogatepass")"""
        return self.update_utf8([t.encode("utf-8", "surrogatepass") for t in texts], **kw)

    def df(self):
        """int32[n_cols]: the document frequencies"""
        out = np.empty(self.n_cols, np.int32)
        _lib.check(self._lib.latok_idf_read(self._open(), _ptr(out), out.size, None))
        return out

    @property
    def n_docs(self):
        n = C.c_int64(0)
        _lib.check(self._lib.latok_idf_info(self._open(), None, C.byref(n), None))
        return n.value

    def weights(self, smooth=True):
        """float32[n_cols]: the idf vector; without smoothing a column with df = 0 gets 0"""
        out = np.empty(self.n_cols, np.float32)
        _lib.check(self._lib.latok_idf_weights(self._open(), 1 if smooth else 0, _ptr(out), out.size))
        return out

    def load(self, df, n_docs):
        """set df and n_docs, for an idf that was fitted elsewhere (or summed over devices); every df[c] must lie in [0, n_docs]"""
        raw = _int32_each(df, self.n_cols, "df", "column")
        _lib.check(self._lib.latok_idf_load(self._open(), _ptr(raw), int(n_docs)))

    def clear(self):
        _lib.check(self._lib.latok_idf_clear(self._open()))


def tfidf_csr(indptr, indices, data, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2"):
    """float32[nnz]: ``TfidfTransformer(norm, use_idf=idf is not None, smooth_idf, sublinear_tf).transform`` of the int32 CSR, weighted
    on the device (``latok_tfidf_csr``): tf (or sign(t)(1 + ln|t|)) times ``idf.weights(smooth_idf)``, over the row's L2 / L1 norm.  A
    row's output bits depend on that row alone."""
    opts, handle = _tfidf_opts(smooth_idf, sublinear_tf, norm), _handle_of(Idf, idf, "idf", True)
    indptr, indices, data, flags = _csr_arrays(indptr, indices, data)
    out = np.empty(data.size, np.float32)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_tfidf_csr(_ptr(indptr), _ptr(indices) if data.size else None, _ptr(data) if data.size else None, indptr.size - 1,
                                   data.size, handle, opts, _ptr(out) if data.size else None, flags, None))
    return out


def _tfidf_rows(utf8, byte_off, vocab, hashed, idf, opts, fold, ng, dtype):
    """the size query, then the fill -> (indptr, indices, data float32, oov or None); folded batches run on device buffers"""
    def entry(b, indptr, oov, indices, data, cap, nnz, flags):
        if hashed:
            seed, n_features, alternate_sign = hashed
            return b.lib.latok_hashed_tfidf_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, seed, n_features, 1 if alternate_sign else 0, ng[0],
                                                             ng[1], ng[2], idf, opts, indptr, indices, data, cap, C.byref(nnz), flags, None)
        return b.lib.latok_tfidf_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, vocab, ng[0], ng[1], ng[2], idf, opts, indptr, oov, indices, data,
                                                  cap, C.byref(nnz), flags, None)

    return _rows_csr(utf8, byte_off, fold, dtype, hashed, np.float32, entry)


def _tfidf_ng(ngram_range, sep):
    return _ngram_spec(ngram_range, sep) or (1, 1, _sep_byte(sep))


def tfidf_utf8_csr(utf8, byte_off, vocab, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2", fold=0, ngram_range=(1, 1), sep=b" ",
                   dtype=np.int64):
    """(indptr, indices int32, data float32, oov): the rows of term_counts_utf8_csr with the same ``vocab`` / ``ngram_range`` / ``sep``,
    their data weighted as tfidf_csr weights it, in one call on the device (``latok_tfidf_utf8_bytes_batch``) -- what
    ``TfidfVectorizer(vocabulary=...).transform`` returns.  ``idf``: an Idf or None (no idf); ``fold``: FOLD_* flags, folded on the device
    first."""
    opts = _tfidf_opts(smooth_idf, sublinear_tf, norm)
    return _tfidf_rows(utf8, byte_off, _handle_of(Vocab, vocab, "vocab"), None, _handle_of(Idf, idf, "idf", True), opts, _fold_bits(fold),
                       _tfidf_ng(ngram_range, sep), dtype)


def tfidf_utf8_batch(blobs, vocab, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2", fold=0, ngram_range=(1, 1), sep=b" "):
    """list[bytes] (UTF-8) -> (indptr, indices, data float32, oov) of tfidf_utf8_csr, int64"""
    utf8, byte_off = pack_utf8(blobs)
    return tfidf_utf8_csr(utf8, byte_off, vocab, idf, smooth_idf, sublinear_tf, norm, fold, ngram_range, sep)


def tfidf_batch(texts, vocab, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2", fold=0, ngram_range=(1, 1), sep=b" "):
    """list[str] -> (indptr, indices, data float32, oov): tfidf_utf8_batch of the strings' UTF-8 ("surrogatepass")"""
    return tfidf_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], vocab, idf, smooth_idf, sublinear_tf, norm, fold, ngram_range, sep)


def hashed_tfidf_utf8_csr(utf8, byte_off, n_features=1 << 20, seed=0, alternate_sign=True, idf=None, smooth_idf=True, sublinear_tf=False,
                          norm="l2", fold=0, ngram_range=(1, 1), sep=b" ", dtype=np.int64):
    """(indptr, indices int32, data float32): the rows of hashed_term_counts_utf8_csr, weighted as tfidf_csr weights them, in one call
    on the device (``latok_hashed_tfidf_utf8_bytes_batch``); without an idf and with norm="l2" this is ``HashingVectorizer``'s own
    default.  An ``idf`` must have ``n_features`` columns."""
    opts, hashed = _tfidf_opts(smooth_idf, sublinear_tf, norm), (_seed32(seed), _n_features31(n_features), bool(alternate_sign))
    return _tfidf_rows(utf8, byte_off, None, hashed, _handle_of(Idf, idf, "idf", True), opts, _fold_bits(fold), _tfidf_ng(ngram_range, sep), dtype)[:3]


def hashed_tfidf_utf8_batch(blobs, n_features=1 << 20, seed=0, alternate_sign=True, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2",
                            fold=0, ngram_range=(1, 1), sep=b" "):
    """list[bytes] (UTF-8) -> (indptr, indices, data float32) of hashed_tfidf_utf8_csr, int64"""
    utf8, byte_off = pack_utf8(blobs)
    return hashed_tfidf_utf8_csr(utf8, byte_off, n_features, seed, alternate_sign, idf, smooth_idf, sublinear_tf, norm, fold, ngram_range, sep)


def hashed_tfidf_batch(texts, n_features=1 << 20, seed=0, alternate_sign=True, idf=None, smooth_idf=True, sublinear_tf=False, norm="l2", fold=0,
                       ngram_range=(1, 1), sep=b" "):
    """list[str] -> (indptr, indices, data float32): hashed_tfidf_utf8_batch of the strings' UTF-8 ("surrogatepass")"""
    return hashed_tfidf_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], n_features, seed, alternate_sign, idf, smooth_idf,
                                   sublinear_tf, norm, fold, ngram_range, sep)


# WordPiece: every token cut greedily into the longest vocabulary prefix and ##-continuations, on the device -- the subword ids a
# BERT-family model takes, as CSR rows or as the padded [n, L] block
class WordPiece(_DeviceObject):
    """A WordPiece vocabulary on the device of the current context (``latok_wordpiece_create``): ``words`` is a list of ``bytes`` or
    ``str`` (``str`` is encoded as UTF-8 with surrogatepass), ``ids`` an optional int32 per word (default: its index), ``prefix``
    the continuation prefix (0 .. 8 bytes, ``##`` in BERT's files), ``max_chars`` BERT's ``max_input_chars_per_word`` (1 .. 1024:
    a token of more chars is one unknown piece), ``seed`` the 32-bit seed of the tables' hash.  Of a duplicate word the first wins.
    Bytes are compared verbatim: the object itself does no lower-casing and no accent stripping.  An uncased vocabulary
    (``bert-base-uncased``) is served by the ``fold=FOLD_UNCASED`` keyword of the ``wordpiece_*`` calls, which folds the batch on the
    device first (``fold_utf8_batch``; fold the words the same way if the file is not folded already).  Still out of scope: the
    punctuation split of BERT's BasicTokenizer (tokens are latok's), the final-sigma rule, a flow form and
    sentence pairs; byte-level BPE is a class of its own, ``BPE``.  Immutable; ``len()`` is the number of words given.  Freed by ``close()``, on leaving a ``with`` block, or with the object."""

    _destroy, _closed = "latok_wordpiece_destroy", "wp must be an open latok_amd.batch.WordPiece"

    def __init__(self, words, ids=None, prefix=b"##", max_chars=100, seed=0):
        seed = _seed32(seed)
        prefix = prefix.encode("utf-8") if isinstance(prefix, str) else bytes(prefix)
        if len(prefix) > 8:
            raise ValueError("prefix must be 0 .. 8 bytes")
        if not isinstance(max_chars, (int, np.integer)) or isinstance(max_chars, bool) or not 1 <= int(max_chars) <= 1024:
            raise ValueError("max_chars must be an int in 1 .. 1024")
        data, off, ids = _pack_words(words, ids)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        pre = np.frombuffer(prefix + b"\x00", np.uint8)
        _lib.check(lib.latok_wordpiece_create(_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(ids) if ids is not None else None,
                                              _ptr(pre), len(prefix), int(max_chars), seed, C.byref(h)))
        self._lib, self.handle, self.seed, self._n = lib, h, seed, off.size - 1
        self.prefix, self.max_chars = prefix, int(max_chars)

    @classmethod
    def from_vocab_file(cls, path, **kw):
        """a BERT ``vocab.txt``: one word per line (UTF-8), id = line number from 0"""
        with open(path, "rb") as f:
            words = [line.rstrip(b"\r\n") for line in f.read().split(b"\n")]
        if words and words[-1] == b"":
            words.pop()                                   # (the file's last newline ends the last word, it starts none)
        return cls(words, **kw)

    def info(self):
        """dict of what ``latok_wordpiece_info`` reports"""
        v = [C.c_int64(0) for _ in range(5)]
        pre, plen, mc, seed, dev = np.zeros(8, np.uint8), C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_int(0)
        _lib.check(self._lib.latok_wordpiece_info(self._open(), *[C.byref(x) for x in v], _ptr(pre), C.byref(plen), C.byref(mc),
                                                  C.byref(seed), C.byref(dev)))
        return dict(n_words=v[0].value, n_slots_initial=v[1].value, n_slots_cont=v[2].value, max_len_initial=v[3].value,
                    max_len_cont=v[4].value, prefix=pre[:plen.value].tobytes(), max_chars=mc.value, seed=seed.value, device=dev.value)

    def __len__(self):
        return self._n


def _wordpiece_ids(utf8, byte_off, wp, unk_id, dtype, spans, fold=0):
    """the size query, then the fill -> (indptr, ids, spans or None) of the batch, or (``fold``) of its folded image"""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    unk_id = _unk32(unk_id)
    dt, flags = _out_dtype(dtype)
    handle = _handle_of(WordPiece, wp, "wp")
    with _batch_on(utf8, byte_off, fold) as b:
        indptr, n = b.out(b.n_str + 1, dt, True), C.c_int64(0)

        def call(ids=None, sp=None, cap=0):
            return b.lib.latok_wordpiece_ids_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, handle, unk_id, _arg(indptr), ids, sp, cap, C.byref(n),
                                                              None, flags | b.flags, None)

        _, (ids, sp) = _size_then_fill(call, n, lambda k: (b.out(k, np.int32), b.out((k, 2), dt) if spans else None))
        return b.fetch(indptr), b.fetch(ids), (b.fetch(sp) if spans else None)


def wordpiece_ids_utf8_csr(utf8, byte_off, wp, unk_id=-1, dtype=np.int64, spans=True):
    """(indptr[n + 1], ids int32[n_pieces], spans[n_pieces, 2] or None): the WordPiece ids of every string -- each token (the byte
    slices token_spans_utf8_bytes_csr reports) cut greedily into the longest word of ``wp`` and ``prefix``-continuations, or ONE
    ``unk_id`` piece when a part of it matches nothing or it has more than ``max_chars`` chars.  spans[r] = piece r's byte range
    inside its string.  indptr and spans in ``dtype``.  Cut and looked up on the device (``latok_wordpiece_ids_utf8_bytes_batch``):
    the size query, then the fill."""
    return _wordpiece_ids(utf8, byte_off, wp, unk_id, dtype, spans)


def wordpiece_ids_utf8_batch(blobs, wp, unk_id=-1, fold=0):
    """list[bytes] (UTF-8) -> (indptr, ids, spans) of wordpiece_ids_utf8_csr, int64 ('' and whitespace-only -> empty rows).  ``fold``
    (FOLD_* flags, ``FOLD_UNCASED`` for an uncased vocabulary): the batch is uploaded once, folded on the device
    (fold_utf8_batch) and cut there; the spans are then byte ranges of the FOLDED string, not of the input."""
    unk_id, fold = _unk32(unk_id), _fold_bits(fold)
    _handle_of(WordPiece, wp, "wp")
    utf8, byte_off = pack_utf8(blobs)
    return _wordpiece_ids(utf8, byte_off, wp, unk_id, np.int64, True, fold)


def wordpiece_ids_batch(texts, wp, unk_id=-1, fold=0):
    """list[str] -> (indptr, ids, spans): wordpiece_ids_utf8_batch of the strings' UTF-8 ("surrogatepass"); the spans are in bytes
    (with ``fold``: bytes of the folded string)."""
    return wordpiece_ids_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], wp, unk_id, fold)


def wordpiece_encode_utf8_batch(blobs, wp, max_length, cls_id=None, sep_id=None, pad_id=0, unk_id=-1, fold=0):
    """list[bytes] (UTF-8) -> (input_ids int32[n, max_length], attention_mask int32[n, max_length]): what a BERT-family model takes.
    Row s = ``cls_id``, the first pieces of string s, ``sep_id``, then ``pad_id``; the two specials are added when BOTH are given
    and omitted when both are None.  A longer row is truncated to ``max_length`` cells, specials included.  attention_mask is 1 on
    the cells in front of the padding.  One call of ``latok_wordpiece_padded_utf8_bytes_batch``; with ``fold`` (FOLD_* flags,
    ``FOLD_UNCASED`` for an uncased vocabulary) behind one call of ``latok_fold_utf8_bytes_batch``, both on device memory."""
    unk_id, pad_id, fold = _unk32(unk_id), _unk32(pad_id), _fold_bits(fold)
    if (cls_id is None) != (sep_id is None):
        raise ValueError("cls_id and sep_id go together: give both or neither")
    special = cls_id is not None
    cls_id, sep_id = (_unk32(cls_id), _unk32(sep_id)) if special else (0, 0)
    if not isinstance(max_length, (int, np.integer)) or isinstance(max_length, bool) or not 1 + 2 * special <= int(max_length) <= 0x7FFFFFFF:
        raise ValueError("max_length must be an int >= %d" % (1 + 2 * special))
    handle = _handle_of(WordPiece, wp, "wp")
    utf8, byte_off = pack_utf8(blobs)
    n_str, max_length = len(blobs), int(max_length)
    with _batch_on(utf8, byte_off, fold if n_str > 0 else 0) as b:   # (an empty list needs no device buffers)
        input_ids, lengths = b.out((n_str, max_length), np.int32), b.out(n_str, np.int32, True)
        _lib.check(b.lib.latok_wordpiece_padded_utf8_bytes_batch(b.u8, b.off, n_str, b.total, handle, unk_id, max_length, 1 if special else 0, cls_id,
                                                                 sep_id, pad_id, _arg(input_ids), _arg(lengths), None, b.flags, None))
        input_ids, lengths = b.fetch(input_ids), b.fetch(lengths)
    mask = (np.arange(max_length, dtype=np.int32)[None, :] < lengths[:, None]).astype(np.int32)
    return input_ids, mask


# byte-level BPE: every token cut by the merge ranks of a GPT-family vocabulary, on the device -- as CSR rows or as the padded [n, L] block
class BPE(_DeviceObject):
    """A byte-level BPE vocabulary on the device of the current context (``latok_bpe_create``): ``words`` is the list of ``bytes`` (or
    ``str``, encoded as UTF-8 with surrogatepass) in RANK order -- a word's rank is its position, of a duplicate the first wins --,
    ``ids`` an optional int32 per word (default: its rank), ``max_bytes`` in 1 .. 4096 (a longer token is one unknown piece),
    ``lead_space``: a token that follows a 0x20 byte inside its string takes that byte in front (the ``" word"`` convention of
    GPT-style vocabularies), ``seed`` the 32-bit seed of the table's hash.  This is ``tiktoken``'s model.  ``pretokenizer`` says what
    cuts the text into the tokens that are merged: ``"latok"`` (the library's tokens; runs of whitespace are not encoded) or ``"gpt2"``
    (GPT-2's regex pre-tokenizer on the device: the ids ``GPT2TokenizerFast`` gives; it carries the space itself, so ``lead_space``
    must be off) or ``"cl100k"`` (the cl100k_base / Llama 3 pattern, likewise).  ``from_gpt2_files`` loads a ``vocab.json`` /
    ``merges.txt`` pair, ``from_tokenizer_json`` a Hugging Face ``tokenizer.json``.  SentencePiece BPE (Llama 2, Mistral: characters
    merged, U+2581 for spaces, byte fallback) is another kind of object of the same class: ``BPE.sentencepiece``,
    ``from_sentencepiece_model`` (a ``tokenizer.model``), ``from_spm_tokenizer_json``.  Out of scope: special-token strings inside the
    text, a ``fold=`` keyword, a flow form, ``DevicePool`` forms, decoding (a class of its own, ``Detokenizer``).  Immutable; ``len()``
    is the number of words given.  Freed by ``close()``, on leaving a ``with`` block, or with the object."""

    _destroy, _closed = "latok_bpe_destroy", "bpe must be an open latok_amd.batch.BPE"

    def __init__(self, words, ids=None, max_bytes=4096, lead_space=False, seed=0, pretokenizer="latok"):
        seed = _seed32(seed)
        if not isinstance(max_bytes, (int, np.integer)) or isinstance(max_bytes, bool) or not 1 <= int(max_bytes) <= 4096:
            raise ValueError("max_bytes must be an int in 1 .. 4096")
        if not isinstance(lead_space, (bool, np.bool_)) and lead_space not in (0, 1):
            raise ValueError("lead_space must be a bool")
        code = _pretok_code(pretokenizer)
        if code == _lib.PRETOK_SPM:
            raise ValueError("pretokenizer='spm' belongs to SentencePiece BPE objects: use BPE.sentencepiece, from_sentencepiece_model or "
                             "from_spm_tokenizer_json (byte merges over these segments mean nothing)")
        if code != _lib.PRETOK_LATOK and lead_space:
            raise ValueError("lead_space must be off with pretokenizer=%r: the space is already in the pre-token" % pretokenizer)
        data, off, ids = _pack_words(words, ids)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        lead = [_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(ids) if ids is not None else None, int(max_bytes), 1 if lead_space else 0]
        if code == _lib.PRETOK_LATOK:
            _lib.check(lib.latok_bpe_create(*lead, seed, C.byref(h)))
        else:
            _lib.check(lib.latok_bpe_create_pretok(*lead, code, seed, C.byref(h)))
        self._lib, self.handle, self.seed, self._n = lib, h, seed, off.size - 1
        self.max_bytes, self.lead_space, self.pretokenizer, self.specials = int(max_bytes), bool(lead_space), pretokenizer, {}

    @classmethod
    def from_tiktoken_file(cls, path, **kw):
        """a ``.tiktoken`` file: lines of ``base64(token) rank``.  The lines are sorted by rank; a line's rank must then equal its
        position, else ValueError."""
        import base64
        pairs = []
        with open(path, "rb") as f:
            for line in f.read().splitlines():
                if not line.strip():
                    continue
                fields = line.split()
                if len(fields) != 2:
                    raise ValueError("a line of a .tiktoken file is `base64(token) rank`: %r" % line[:60])
                try:
                    pairs.append((int(fields[1]), base64.b64decode(fields[0], validate=True)))
                except Exception:
                    raise ValueError("a line of a .tiktoken file is `base64(token) rank`: %r" % line[:60]) from None
        pairs.sort(key=lambda p: p[0])
        for i, (rank, _) in enumerate(pairs):
            if rank != i:
                raise ValueError("the ranks of a .tiktoken file must be 0 .. n - 1, each once: position %d holds rank %d" % (i, rank))
        return cls([w for _, w in pairs], **kw)

    @staticmethod
    def gpt2_byte_decoder():
        """dict: the printable character GPT-2 writes for a byte in vocab.json and merges.txt -> that byte (its ``bytes_to_unicode``, inverted)"""
        keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
        table, n = {chr(b): b for b in keep}, 0
        for b in range(256):
            if b not in keep:
                table[chr(256 + n)] = b
                n += 1
        return table

    @staticmethod
    def gpt2_word_list(vocab_json, merges_txt):
        """(words, ids, specials) of a GPT-2 ``vocab.json`` / ``merges.txt`` pair; needs no device.  ``words``: the single bytes that
        vocab.json holds, in byte order, then the result of every merge in the file's order, which is the rank order; ``ids``: theirs in
        vocab.json.  An entry of vocab.json that is neither is a special token: it is NOT made a word (the whole-token shortcut would
        match its literal text) and goes to ``specials`` (name -> id).  A merge result that vocab.json lacks is a ValueError."""
        import json
        with open(vocab_json, encoding="utf-8") as f:
            vocab = json.load(f)
        if not isinstance(vocab, dict) or not all(isinstance(k, str) and isinstance(v, int) and not isinstance(v, bool) for k, v in vocab.items()):
            raise ValueError("vocab.json must be one object of token -> id")
        dec = BPE.gpt2_byte_decoder()

        def raw(token, where):
            try:
                return bytes(dec[ch] for ch in token)
            except KeyError:
                raise ValueError("%s: %r is not written in GPT-2's byte alphabet" % (where, token[:40])) from None

        enc = {b: ch for ch, b in dec.items()}
        words, ids, used = [], [], set()
        for b in range(256):
            if enc[b] in vocab:
                words.append(bytes([b]))
                ids.append(vocab[enc[b]])
                used.add(enc[b])
        with open(merges_txt, encoding="utf-8") as f:
            for no, line in enumerate(f.read().split("\n"), 1):
                if not line.strip() or (no == 1 and line.startswith("#version")):
                    continue
                pair = line.split(" ")
                if len(pair) != 2 or not pair[0] or not pair[1]:
                    raise ValueError("merges.txt line %d is not `left right`: %r" % (no, line[:60]))
                token = pair[0] + pair[1]
                if token not in vocab:
                    raise ValueError("merges.txt line %d: the merge result %r is not in vocab.json" % (no, token[:40]))
                words.append(raw(token, "merges.txt line %d" % no))
                ids.append(vocab[token])
                used.add(token)
        specials = {k: v for k, v in vocab.items() if k not in used}
        return words, ids, specials

    @classmethod
    def from_gpt2_files(cls, vocab_json, merges_txt, pretokenizer="gpt2", **kw):
        """GPT-2's own files (also RoBERTa's and BART's): ``gpt2_word_list`` of the pair, cut by ``pretokenizer``.  The special tokens of
        vocab.json are in the ``specials`` attribute (name -> id); they are not recognised inside text."""
        words, ids, specials = cls.gpt2_word_list(vocab_json, merges_txt)
        self = cls(words, ids=ids, pretokenizer=pretokenizer, **kw)
        self.specials = specials
        return self

    # the cl100k / Llama 3 pattern as a tokenizer.json spells it
    CL100K_PATTERN = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+"
                      r"|\s+(?!\S)|\s+")

    @staticmethod
    def _tokenizer_json_pretokenizer(pre):
        """the pre-tokenizer name of a tokenizer.json's ``pre_tokenizer`` entry: recognised, never guessed"""
        def byte_level(p, use_regex):
            if p.get("add_prefix_space"):
                raise ValueError("tokenizer.json: add_prefix_space is not supported")
            return p.get("type") == "ByteLevel" and bool(p.get("use_regex", True)) == use_regex

        if isinstance(pre, dict) and pre.get("type") == "ByteLevel" and byte_level(pre, True):
            return "gpt2"
        if isinstance(pre, dict) and pre.get("type") == "Sequence":
            steps = pre.get("pretokenizers")
            if isinstance(steps, list) and len(steps) == 2 and all(isinstance(p, dict) for p in steps):
                split, level = steps
                if (split.get("type") == "Split" and split.get("pattern") == {"Regex": BPE.CL100K_PATTERN} and not split.get("invert")
                        and str(split.get("behavior")).lower() == "isolated" and level.get("type") == "ByteLevel" and byte_level(level, False)):
                    return "cl100k"
        import json
        raise ValueError("tokenizer.json: the pre_tokenizer is neither ByteLevel with its regex (gpt2) nor Split by the cl100k pattern "
                         "followed by ByteLevel without it (cl100k): %s" % json.dumps(pre)[:300])

    @staticmethod
    def tokenizer_json_word_list(path):
        """(words, ids, specials, pretokenizer) of a Hugging Face ``tokenizer.json`` whose model is byte-level BPE; needs no device.
        ``words``, ``ids`` and ``specials`` follow ``gpt2_word_list``: the single bytes of the vocabulary in byte order, then the result of
        every merge in the file's order (a merge is ``"left right"`` or a pair); the ``added_tokens`` and whatever else the vocabulary
        holds are ``specials`` (content -> id), never words.  ``pretokenizer`` is ``"gpt2"`` or ``"cl100k"``, read off the file's
        ``pre_tokenizer``; anything else there, a normalizer, ``add_prefix_space`` or another model is a ValueError that names it."""
        import json
        with open(path, encoding="utf-8") as f:
            tj = json.load(f)
        model = tj.get("model") if isinstance(tj, dict) else None
        if not isinstance(model, dict) or model.get("type", "BPE") != "BPE" or not isinstance(model.get("vocab"), dict) or not isinstance(model.get("merges"), list):
            raise ValueError("tokenizer.json: the model is not BPE with a vocab and merges: %r" % (model.get("type") if isinstance(model, dict) else model,))
        for key in ("byte_fallback", "dropout", "continuing_subword_prefix", "end_of_word_suffix"):
            if model.get(key):
                raise ValueError("tokenizer.json: the model's %s (%r) is not supported" % (key, model[key]))
        if tj.get("normalizer") is not None:
            raise ValueError("tokenizer.json: a normalizer is not supported: %s" % json.dumps(tj["normalizer"])[:200])
        pretokenizer = BPE._tokenizer_json_pretokenizer(tj.get("pre_tokenizer"))
        vocab = model["vocab"]
        if not all(isinstance(k, str) and isinstance(v, int) and not isinstance(v, bool) for k, v in vocab.items()):
            raise ValueError("tokenizer.json: the vocab must be one object of token -> id")
        dec = BPE.gpt2_byte_decoder()
        enc = {b: ch for ch, b in dec.items()}
        words, ids, used = [], [], set()
        for b in range(256):
            if enc[b] in vocab:
                words.append(bytes([b]))
                ids.append(vocab[enc[b]])
                used.add(enc[b])
        for no, merge in enumerate(model["merges"], 1):
            pair = merge.split(" ") if isinstance(merge, str) else merge
            if not isinstance(pair, list) or len(pair) != 2 or not all(isinstance(x, str) and x for x in pair):
                raise ValueError("tokenizer.json: merge %d is not `left right`: %r" % (no, merge))
            token = pair[0] + pair[1]
            if token not in vocab:
                raise ValueError("tokenizer.json: merge %d: the merge result %r is not in the vocab" % (no, token[:40]))
            try:
                words.append(bytes(dec[ch] for ch in token))
            except KeyError:
                raise ValueError("tokenizer.json: merge %d: %r is not written in GPT-2's byte alphabet" % (no, token[:40])) from None
            ids.append(vocab[token])
            used.add(token)
        specials = {k: v for k, v in vocab.items() if k not in used}
        for a in tj.get("added_tokens") or []:
            if not isinstance(a, dict) or not isinstance(a.get("content"), str) or not isinstance(a.get("id"), int):
                raise ValueError("tokenizer.json: an added token is not {id, content}: %r" % (a,))
            specials[a["content"]] = a["id"]
        return words, ids, specials, pretokenizer

    @classmethod
    def from_tokenizer_json(cls, path, **kw):
        """a Hugging Face ``tokenizer.json`` with a byte-level BPE model (GPT-2's, Llama 3's, ...): ``tokenizer_json_word_list`` of it, cut
        by the pre-tokenizer the file names (``pretokenizer=`` overrides it).  The added tokens are in the ``specials`` attribute (content
        -> id); they are not recognised inside text."""
        words, ids, specials, pretokenizer = cls.tokenizer_json_word_list(path)
        kw.setdefault("pretokenizer", pretokenizer)
        self = cls(words, ids=ids, **kw)
        self.specials = specials
        return self

    # ---- SentencePiece BPE (latok_bpe_create_spm): Llama 2, Mistral, ... -----------------------------------------------------------------
    @classmethod
    def sentencepiece(cls, words, ids=None, byte_ids=None, add_dummy_prefix=True, fuse_unk=True, max_bytes=4096, seed=0):
        """A SentencePiece BPE vocabulary on the device (``latok_bpe_create_spm``): ``words`` in RANK order (characters and merge results;
        the marker U+2581 stands for a space), ``ids`` as above, ``byte_ids`` 256 int32 ids of the byte pieces or None (no byte
        fallback: an unknown character is one ``unk_id`` piece, a run of them ONE with ``fuse_unk``), ``add_dummy_prefix``: one marker
        in front of every string.  The text is cut into SentencePiece's segments (``pretokenize_batch(texts, "spm")``), characters are
        merged, there is no whole-segment shortcut.  ``bpe_ids_*`` and ``bpe_encode_*`` take the object as they take any other."""
        seed = _seed32(seed)
        if not isinstance(max_bytes, (int, np.integer)) or isinstance(max_bytes, bool) or not 1 <= int(max_bytes) <= 4096:
            raise ValueError("max_bytes must be an int in 1 .. 4096")
        for name, flag in (("add_dummy_prefix", add_dummy_prefix), ("fuse_unk", fuse_unk)):
            if not isinstance(flag, (bool, np.bool_)) and flag not in (0, 1):
                raise ValueError("%s must be a bool" % name)
        if byte_ids is not None:
            byte_ids = _int32_each(byte_ids, 256, "byte_ids", "byte")
        data, off, ids = _pack_words(words, ids)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        _lib.check(lib.latok_bpe_create_spm(_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(ids) if ids is not None else None,
                                            _ptr(byte_ids) if byte_ids is not None else None, 1 if add_dummy_prefix else 0, 1 if fuse_unk else 0,
                                            int(max_bytes), seed, C.byref(h)))
        self = cls.__new__(cls)
        self._lib, self.handle, self.seed, self._n = lib, h, seed, off.size - 1
        self.max_bytes, self.lead_space, self.pretokenizer, self.specials = int(max_bytes), False, "spm", {}
        self.byte_fallback, self.add_dummy_prefix, self.fuse_unk = byte_ids is not None, bool(add_dummy_prefix), bool(fuse_unk)
        return self

    @staticmethod
    def _proto_fields(buf):
        """the fields of one protobuf message: (number, wire type, value) -- varint and fixed values as ints, length-delimited as bytes"""
        i, n = 0, len(buf)

        def varint():
            nonlocal i
            v = shift = 0
            while True:
                if i >= n or shift > 63:
                    raise ValueError("not a SentencePiece model: a varint runs out of the message")
                b = buf[i]
                i += 1
                v |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    return v

        while i < n:
            key = varint()
            no, wt = key >> 3, key & 7
            if wt == 0:
                yield no, wt, varint()
            elif wt in (1, 5):
                size = 8 if wt == 1 else 4
                if i + size > n:
                    raise ValueError("not a SentencePiece model: a fixed field runs out of the message")
                yield no, wt, int.from_bytes(buf[i:i + size], "little")
                i += size
            elif wt == 2:
                size = varint()
                if i + size > n:
                    raise ValueError("not a SentencePiece model: a field runs out of the message")
                yield no, wt, bytes(buf[i:i + size])
                i += size
            else:
                raise ValueError("not a SentencePiece model: wire type %d" % wt)

    @staticmethod
    def read_sentencepiece_model(path):
        """what a ``tokenizer.model`` (a serialized ``ModelProto``) says, by a reader of the wire format of its own -- no ``protobuf``, no
        ``sentencepiece``: dict of ``pieces`` [(bytes, score, type)] in id order, ``model_type``, ``byte_fallback``,
        ``treat_whitespace_as_suffix``, ``normalizer_name``, ``charsmap`` (bytes), ``add_dummy_prefix``, ``remove_extra_whitespaces``,
        ``escape_whitespaces``.  Field numbers as in sentencepiece_model.proto; absent fields take the proto's defaults."""
        import struct
        with open(path, "rb") as f:
            buf = f.read()
        m = dict(pieces=[], model_type=1, byte_fallback=False, treat_whitespace_as_suffix=False, normalizer_name="", charsmap=b"",
                 add_dummy_prefix=True, remove_extra_whitespaces=True, escape_whitespaces=True)
        for no, wt, v in BPE._proto_fields(buf):
            if no == 1 and wt == 2:                      # repeated SentencePiece pieces = 1
                piece, score, kind = b"", 0.0, 1
                for n2, w2, v2 in BPE._proto_fields(v):
                    if n2 == 1 and w2 == 2:
                        piece = v2
                    elif n2 == 2 and w2 == 5:
                        score = struct.unpack("<f", v2.to_bytes(4, "little"))[0]
                    elif n2 == 3 and w2 == 0:
                        kind = v2
                m["pieces"].append((piece, score, kind))
            elif no == 2 and wt == 2:                    # TrainerSpec trainer_spec = 2
                for n2, w2, v2 in BPE._proto_fields(v):
                    if n2 == 3 and w2 == 0:
                        m["model_type"] = v2
                    elif n2 == 35 and w2 == 0:
                        m["byte_fallback"] = bool(v2)
                    elif n2 == 24 and w2 == 0:
                        m["treat_whitespace_as_suffix"] = bool(v2)
            elif no == 3 and wt == 2:                    # NormalizerSpec normalizer_spec = 3
                for n2, w2, v2 in BPE._proto_fields(v):
                    if n2 == 1 and w2 == 2:
                        m["normalizer_name"] = v2.decode("utf-8", "replace")
                    elif n2 == 2 and w2 == 2:
                        m["charsmap"] = v2
                    elif n2 == 3 and w2 == 0:
                        m["add_dummy_prefix"] = bool(v2)
                    elif n2 == 4 and w2 == 0:
                        m["remove_extra_whitespaces"] = bool(v2)
                    elif n2 == 5 and w2 == 0:
                        m["escape_whitespaces"] = bool(v2)
        if not m["pieces"]:
            raise ValueError("not a SentencePiece model: it holds no piece")
        return m

    @staticmethod
    def sentencepiece_word_list(path):
        """(words, ids, byte_ids, specials, add_dummy_prefix) of a SentencePiece ``tokenizer.model`` of type BPE; needs no device.
        ``words``: the NORMAL pieces sorted by score descending, stable in id order, ``ids`` theirs in the file; ``byte_ids``: the ids
        of the 256 BYTE pieces, or None without ``byte_fallback``; ``specials``: the CONTROL and UNKNOWN pieces (name -> id).  A
        ValueError names whatever the device rule does not cover: another model type, a normalizer other than ``identity`` with an empty
        charsmap, ``remove_extra_whitespaces``, no ``escape_whitespaces``, whitespace as suffix, USER_DEFINED or UNUSED pieces, fewer
        than 256 byte pieces under ``byte_fallback``."""
        m = BPE.read_sentencepiece_model(path)
        if m["model_type"] != 2:
            raise ValueError("SentencePiece model: model_type is %s, not BPE" % {1: "UNIGRAM", 3: "WORD", 4: "CHAR"}.get(m["model_type"], m["model_type"]))
        if m["normalizer_name"] != "identity" or m["charsmap"]:
            raise ValueError("SentencePiece model: the normalizer is %r with a charsmap of %d bytes; only `identity` with an empty charsmap is "
                             "supported" % (m["normalizer_name"], len(m["charsmap"])))
        if m["remove_extra_whitespaces"]:
            raise ValueError("SentencePiece model: remove_extra_whitespaces is not supported")
        if not m["escape_whitespaces"]:
            raise ValueError("SentencePiece model: escape_whitespaces must be on")
        if m["treat_whitespace_as_suffix"]:
            raise ValueError("SentencePiece model: treat_whitespace_as_suffix is not supported")
        normal, specials, by_byte = [], {}, {}
        for pid, (piece, score, kind) in enumerate(m["pieces"]):
            if kind == 1:
                normal.append((piece, score, pid))
            elif kind in (2, 3):
                specials[piece.decode("utf-8", "surrogateescape")] = pid
            elif kind == 6:
                name = piece.decode("ascii", "replace")
                if len(name) != 6 or not name.startswith("<0x") or not name.endswith(">"):
                    raise ValueError("SentencePiece model: the BYTE piece %r is not <0xXX>" % name)
                by_byte.setdefault(int(name[3:5], 16), pid)
            else:
                raise ValueError("SentencePiece model: piece %d (%r) is %s; such pieces are not supported"
                                 % (pid, piece[:40], {4: "USER_DEFINED", 5: "UNUSED"}.get(kind, "of type %d" % kind)))
        byte_ids = None
        if m["byte_fallback"]:
            if len(by_byte) != 256:
                raise ValueError("SentencePiece model: byte_fallback with %d of the 256 byte pieces" % len(by_byte))
            byte_ids = [by_byte[b] for b in range(256)]
        normal.sort(key=lambda t: -t[1])   # (stable: equal scores stay in id order)
        return [t[0] for t in normal], [t[2] for t in normal], byte_ids, specials, m["add_dummy_prefix"]

    @classmethod
    def from_sentencepiece_model(cls, path, **kw):
        """a SentencePiece ``tokenizer.model`` of type BPE (Llama 2, Code Llama, Mistral 7B, Mixtral, TinyLlama, Yi):
        ``sentencepiece_word_list`` of it as a ``BPE.sentencepiece`` object.  The CONTROL and UNKNOWN pieces are in the ``specials``
        attribute (name -> id) and the unknown piece's id in ``unk_id``; they are not recognised inside text."""
        words, ids, byte_ids, specials, dummy = cls.sentencepiece_word_list(path)
        kw.setdefault("add_dummy_prefix", dummy)
        self = cls.sentencepiece(words, ids=ids, byte_ids=byte_ids, **kw)
        self.specials = specials
        self.unk_id = specials.get("<unk>", -1)
        return self

    @staticmethod
    def spm_tokenizer_json_word_list(path):
        """(words, ids, byte_ids, specials, add_dummy_prefix) of a Hugging Face ``tokenizer.json`` that spells a SentencePiece BPE model;
        needs no device.  Accepted: model ``BPE`` with ``byte_fallback: true``; normalizer exactly ``Sequence[Prepend("▁"),
        Replace(" " -> "▁")]`` or the ``Replace`` alone (no dummy prefix); ``pre_tokenizer`` null.  ``words``: the merge results in
        merge order, the first producer winning, then every remaining entry of the vocabulary that is neither ``<0xXX>`` nor an added
        token.  Everything else is a ValueError."""
        import json
        with open(path, encoding="utf-8") as f:
            tj = json.load(f)
        model = tj.get("model") if isinstance(tj, dict) else None
        if not isinstance(model, dict) or model.get("type", "BPE") != "BPE" or not isinstance(model.get("vocab"), dict) or not isinstance(model.get("merges"), list):
            raise ValueError("tokenizer.json: the model is not BPE with a vocab and merges: %r" % (model.get("type") if isinstance(model, dict) else model,))
        if not model.get("byte_fallback"):
            raise ValueError("tokenizer.json: the model has no byte_fallback: not a SentencePiece BPE file (see from_tokenizer_json)")
        for key in ("dropout", "continuing_subword_prefix", "end_of_word_suffix", "ignore_merges"):
            if model.get(key):
                raise ValueError("tokenizer.json: the model's %s (%r) is not supported" % (key, model[key]))
        if tj.get("pre_tokenizer") is not None:
            raise ValueError("tokenizer.json: a pre_tokenizer is not supported here: %s" % json.dumps(tj["pre_tokenizer"])[:200])
        mark = "▁"

        def is_replace(p):
            return isinstance(p, dict) and p.get("type") == "Replace" and p.get("pattern") == {"String": " "} and p.get("content") == mark

        norm = tj.get("normalizer")
        if is_replace(norm):
            dummy = False
        elif (isinstance(norm, dict) and norm.get("type") == "Sequence" and isinstance(norm.get("normalizers"), list) and len(norm["normalizers"]) == 2
              and isinstance(norm["normalizers"][0], dict) and norm["normalizers"][0].get("type") == "Prepend"
              and norm["normalizers"][0].get("prepend") == mark and is_replace(norm["normalizers"][1])):
            dummy = True
        else:
            raise ValueError("tokenizer.json: the normalizer is neither Sequence[Prepend(U+2581), Replace(' ' -> U+2581)] nor that Replace "
                             "alone: %s" % json.dumps(norm)[:300])
        vocab = model["vocab"]
        if not all(isinstance(k, str) and isinstance(v, int) and not isinstance(v, bool) for k, v in vocab.items()):
            raise ValueError("tokenizer.json: the vocab must be one object of token -> id")
        specials = {}
        for a in tj.get("added_tokens") or []:
            if not isinstance(a, dict) or not isinstance(a.get("content"), str) or not isinstance(a.get("id"), int):
                raise ValueError("tokenizer.json: an added token is not {id, content}: %r" % (a,))
            specials[a["content"]] = a["id"]
        if isinstance(model.get("unk_token"), str) and model["unk_token"] in vocab:
            specials.setdefault(model["unk_token"], vocab[model["unk_token"]])
        words, ids, used = [], [], set()
        for no, merge in enumerate(model["merges"], 1):
            pair = merge.split(" ") if isinstance(merge, str) else merge
            if not isinstance(pair, list) or len(pair) != 2 or not all(isinstance(x, str) and x for x in pair):
                raise ValueError("tokenizer.json: merge %d is not `left right`: %r" % (no, merge))
            token = pair[0] + pair[1]
            if token not in vocab:
                raise ValueError("tokenizer.json: merge %d: the merge result %r is not in the vocab" % (no, token[:40]))
            if token in used:
                continue                             # (the first producer wins)
            used.add(token)
            words.append(token.encode("utf-8", "surrogatepass"))
            ids.append(vocab[token])
        by_byte = {}
        for token, pid in vocab.items():
            if len(token) == 6 and token.startswith("<0x") and token.endswith(">"):
                try:
                    by_byte.setdefault(int(token[3:5], 16), pid)
                    continue
                except ValueError:
                    pass
            if token in used or token in specials:
                continue
            words.append(token.encode("utf-8", "surrogatepass"))
            ids.append(pid)
        if len(by_byte) != 256:
            raise ValueError("tokenizer.json: byte_fallback with %d of the 256 <0xXX> entries" % len(by_byte))
        return words, ids, [by_byte[b] for b in range(256)], specials, dummy

    @classmethod
    def from_spm_tokenizer_json(cls, path, **kw):
        """the Hugging Face ``tokenizer.json`` of a SentencePiece BPE model (Llama 2's, Mistral's): ``spm_tokenizer_json_word_list`` of it as
        a ``BPE.sentencepiece`` object; ``specials`` and ``unk_id`` as ``from_sentencepiece_model`` leaves them."""
        words, ids, byte_ids, specials, dummy = cls.spm_tokenizer_json_word_list(path)
        kw.setdefault("add_dummy_prefix", dummy)
        self = cls.sentencepiece(words, ids=ids, byte_ids=byte_ids, **kw)
        self.specials = specials
        self.unk_id = specials.get("<unk>", -1)
        return self

    def spm_info(self):
        """dict of what ``latok_bpe_spm_info`` reports (a SentencePiece object only)"""
        v = [C.c_int(0) for _ in range(3)]
        _lib.check(self._lib.latok_bpe_spm_info(self._open(), *[C.byref(x) for x in v]))
        return dict(byte_fallback=v[0].value, add_dummy_prefix=v[1].value, fuse_unk=v[2].value)

    def info(self):
        """dict of what ``latok_bpe_info`` reports"""
        v = [C.c_int64(0) for _ in range(3)]
        mb, ls, seed, dev = C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_int(0)
        _lib.check(self._lib.latok_bpe_info(self._open(), *[C.byref(x) for x in v], C.byref(mb), C.byref(ls), C.byref(seed), C.byref(dev)))
        return dict(n_words=v[0].value, n_slots=v[1].value, max_len=v[2].value, max_bytes=mb.value, lead_space=ls.value, seed=seed.value,
                    device=dev.value)

    def pretokenizer_of_object(self):
        """the name of what ``latok_bpe_pretokenizer`` reports for the device object"""
        pt = C.c_int(-1)
        _lib.check(self._lib.latok_bpe_pretokenizer(self._open(), C.byref(pt)))
        return {v: k for k, v in _PRETOKENIZERS.items()}[pt.value]

    def __len__(self):
        return self._n


def bpe_ids_utf8_csr(utf8, byte_off, bpe, unk_id=-1, dtype=np.int64, spans=True):
    """(indptr[n + 1], ids int32[n_pieces], spans[n_pieces, 2] or None): the BPE ids of every string -- each token (the byte slices
    token_spans_utf8_bytes_csr reports, with the space in front under ``lead_space``; GPT-2's pre-tokens, the slices of
    pretokens_utf8_csr, when ``bpe`` was made with ``pretokenizer="gpt2"``) is one piece if it is a word of ``bpe``, else
    its bytes merged pair by pair, lowest rank first and leftmost among equals; a byte that is no word is an ``unk_id`` piece, a token of
    more than ``max_bytes`` bytes ONE.  spans[r] = piece r's byte range inside its string.  indptr and spans in ``dtype``.  Cut on the
    device (``latok_bpe_ids_utf8_bytes_batch``): the size query, then the fill."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    unk_id = _unk32(unk_id)
    dt, flags = _out_dtype(dtype)
    handle = _handle_of(BPE, bpe, "bpe")
    with _HostBatch(utf8, byte_off) as b:
        indptr, n = b.out(b.n_str + 1, dt, True), C.c_int64(0)

        def call(ids=None, sp=None, cap=0):
            return b.lib.latok_bpe_ids_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, handle, unk_id, _arg(indptr), ids, sp, cap, C.byref(n), None,
                                                        flags | b.flags, None)

        _, (ids, sp) = _size_then_fill(call, n, lambda k: (b.out(k, np.int32), b.out((k, 2), dt) if spans else None))
        return b.fetch(indptr), b.fetch(ids), (b.fetch(sp) if spans else None)


def bpe_ids_utf8_batch(blobs, bpe, unk_id=-1):
    """list[bytes] (UTF-8) -> (indptr, ids, spans) of bpe_ids_utf8_csr, int64 ('' and whitespace-only -> empty rows)"""
    unk_id = _unk32(unk_id)
    _handle_of(BPE, bpe, "bpe")
    utf8, byte_off = pack_utf8(blobs)
    return bpe_ids_utf8_csr(utf8, byte_off, bpe, unk_id, np.int64, True)


def bpe_ids_batch(texts, bpe, unk_id=-1):
    """list[str] -> (indptr, ids, spans): bpe_ids_utf8_batch of the strings' UTF-8 ("surrogatepass"); the spans are in bytes"""
    return bpe_ids_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], bpe, unk_id)


def bpe_encode_utf8_batch(blobs, bpe, max_length, bos_id=None, eos_id=None, pad_id=0, unk_id=-1):
    """list[bytes] (UTF-8) -> (input_ids int32[n, max_length], attention_mask int32[n, max_length]): what a GPT-family model takes.
    Row s = ``bos_id``, the first pieces of string s, ``eos_id``, then ``pad_id``; the two specials are added when BOTH are given and
    omitted when both are None.  A longer row is truncated to ``max_length`` cells, specials included.  attention_mask is 1 on the
    cells in front of the padding.  One call of ``latok_bpe_padded_utf8_bytes_batch``."""
    unk_id, pad_id = _unk32(unk_id), _unk32(pad_id)
    if (bos_id is None) != (eos_id is None):
        raise ValueError("bos_id and eos_id go together: give both or neither")
    special = bos_id is not None
    bos_id, eos_id = (_unk32(bos_id), _unk32(eos_id)) if special else (0, 0)
    if not isinstance(max_length, (int, np.integer)) or isinstance(max_length, bool) or not 1 + 2 * special <= int(max_length) <= 0x7FFFFFFF:
        raise ValueError("max_length must be an int >= %d" % (1 + 2 * special))
    handle = _handle_of(BPE, bpe, "bpe")
    utf8, byte_off = pack_utf8(blobs)
    n_str, max_length = len(blobs), int(max_length)
    with _HostBatch(utf8, byte_off) as b:
        input_ids, lengths = b.out((n_str, max_length), np.int32), b.out(n_str, np.int32, True)
        _lib.check(b.lib.latok_bpe_padded_utf8_bytes_batch(b.u8, b.off, n_str, b.total, handle, unk_id, max_length, 1 if special else 0, bos_id,
                                                           eos_id, pad_id, _arg(input_ids), _arg(lengths), None, b.flags, None))
        input_ids, lengths = b.fetch(input_ids), b.fetch(lengths)
    mask = (np.arange(max_length, dtype=np.int32)[None, :] < lengths[:, None]).astype(np.int32)
    return input_ids, mask


# Unigram: every token cut by the Viterbi search of a SentencePiece Unigram model, on the device -- as CSR rows or as the padded [n, L] block
class Unigram(_DeviceObject):
    """A Unigram vocabulary on the device of the current context (``latok_unigram_create``): ``words`` is the list of ``bytes`` (or
    ``str``, encoded as UTF-8 with surrogatepass), ``scores`` one finite float32 per word (log probabilities), ``ids`` an optional int32
    per word (default: its position; of a duplicate word the first wins), ``marker`` the 0 .. 4 bytes of ONE character that stand in
    front of a token at a string's start or behind whitespace (SentencePiece's U+2581), ``unk_score`` the score of an unknown
    character (default: ``float32(min(scores)) - 10``, SentencePiece's penalty; -10 for an empty vocabulary), ``fuse_unk``: neighbouring
    unknown pieces of a token become one, ``max_bytes`` in 1 .. 4096 (a longer token is one unknown piece), ``seed`` the 32-bit seed of
    the tables' hash.  The cut is the best-scoring split of ``marker + token`` into words, float32 sums, of equal scores the lower
    start.  Out of scope: SentencePiece's normalizer (tokens are latok's), ``byte_fallback``, sampling, a ``.model`` protobuf loader, a
    ``fold=`` keyword, a flow form, ``DevicePool`` forms, an EOS-only padded layout, turning the marker back into spaces when decoding
    (a ``Detokenizer`` built from the same word list decodes the ids in ``mode="concat"``, the marker in the bytes).  Immutable;
    ``len()`` is the number of words given.  Freed by ``close()``, on leaving a ``with`` block, or with the object."""

    _destroy, _closed = "latok_unigram_destroy", "unigram must be an open latok_amd.batch.Unigram"

    def __init__(self, words, scores, ids=None, marker="\u2581".encode(), unk_score=None, fuse_unk=True, max_bytes=4096, seed=0):
        seed = _seed32(seed)
        if not isinstance(max_bytes, (int, np.integer)) or isinstance(max_bytes, bool) or not 1 <= int(max_bytes) <= 4096:
            raise ValueError("max_bytes must be an int in 1 .. 4096")
        if not isinstance(fuse_unk, (bool, np.bool_)) and fuse_unk not in (0, 1):
            raise ValueError("fuse_unk must be a bool")
        if isinstance(marker, str):
            marker = marker.encode("utf-8", "surrogatepass")
        marker = bytes(marker)
        if len(marker) > 4 or any((b & 0xC0) != 0x80 for b in marker[1:]):
            raise ValueError("marker must be the bytes of one character, 4 at most, or empty")
        data, off, ids = _pack_words(words, ids)
        scores = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
        if scores.size != off.size - 1:
            raise ValueError("scores must hold one float per word")
        if not np.isfinite(scores).all():
            raise ValueError("every score must be finite")
        if unk_score is None:
            unk_score = np.float32(scores.min()) - np.float32(10) if scores.size else np.float32(-10)
        unk_score = np.float32(unk_score)
        if not np.isfinite(unk_score):
            raise ValueError("unk_score must be finite")
        mk = np.frombuffer(marker + b"\0", np.uint8)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        _lib.check(lib.latok_unigram_create(_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(scores) if scores.size else None,
                                            _ptr(ids) if ids is not None else None, _ptr(mk), len(marker), float(unk_score), 1 if fuse_unk else 0,
                                            int(max_bytes), seed, C.byref(h)))
        self._lib, self.handle, self.seed, self._n = lib, h, seed, off.size - 1
        self.marker, self.unk_score, self.fuse_unk, self.max_bytes = marker, float(unk_score), bool(fuse_unk), int(max_bytes)

    @classmethod
    def from_vocab_file(cls, path, **kw):
        """SentencePiece's exported ``.vocab``: one ``piece<TAB>score`` per line, the id is the line's position"""
        words, scores = [], []
        with open(path, "rb") as f:
            for line in f.read().split(b"\n"):
                if not line:
                    continue
                fields = line.rstrip(b"\r").split(b"\t")
                try:
                    if len(fields) != 2:
                        raise ValueError
                    scores.append(float(fields[1]))
                except ValueError:
                    raise ValueError("a line of a .vocab file is `piece<TAB>score`: %r" % line[:60]) from None
                words.append(fields[0])
        return cls(words, scores, **kw)

    def info(self):
        """dict of what ``latok_unigram_info`` reports"""
        v = [C.c_int64(0) for _ in range(5)]
        mk = np.zeros(4, np.uint8)
        ml, us, fu, mb, seed, dev = C.c_int(0), C.c_float(0), C.c_int(0), C.c_int(0), C.c_uint32(0), C.c_int(0)
        _lib.check(self._lib.latok_unigram_info(self._open(), *[C.byref(x) for x in v], _ptr(mk), C.byref(ml), C.byref(us), C.byref(fu), C.byref(mb),
                                                C.byref(seed), C.byref(dev)))
        return dict(n_words=v[0].value, n_slots_plain=v[1].value, n_slots_marked=v[2].value, max_len=v[3].value, marker_word=v[4].value,
                    marker=mk.tobytes()[:ml.value], unk_score=us.value, fuse_unk=fu.value, max_bytes=mb.value, seed=seed.value, device=dev.value)

    def __len__(self):
        return self._n


def unigram_ids_utf8_csr(utf8, byte_off, unigram, unk_id=-1, dtype=np.int64, spans=True):
    """(indptr[n + 1], ids int32[n_pieces], spans[n_pieces, 2] or None): the Unigram ids of every string -- each token (the byte slices
    token_spans_utf8_bytes_csr reports, the marker in front of it at a string's start and behind whitespace) is cut into the words of
    ``unigram`` with the highest float32 score sum; a character that is no word is an ``unk_id`` piece (neighbours fused under
    ``fuse_unk``), a token of more than ``max_bytes`` bytes ONE.  spans[r] = piece r's byte range inside its string (empty for the
    marker alone).  indptr and spans in ``dtype``.  Cut on the device (``latok_unigram_ids_utf8_bytes_batch``): the size query, then the fill."""
    utf8, byte_off = _csr_u8(utf8, byte_off)
    unk_id = _unk32(unk_id)
    dt, flags = _out_dtype(dtype)
    handle = _handle_of(Unigram, unigram, "unigram")
    with _HostBatch(utf8, byte_off) as b:
        indptr, n = b.out(b.n_str + 1, dt, True), C.c_int64(0)

        def call(ids=None, sp=None, cap=0):
            return b.lib.latok_unigram_ids_utf8_bytes_batch(b.u8, b.off, b.n_str, b.total, handle, unk_id, _arg(indptr), ids, sp, cap, C.byref(n), None,
                                                            flags | b.flags, None)

        _, (ids, sp) = _size_then_fill(call, n, lambda k: (b.out(k, np.int32), b.out((k, 2), dt) if spans else None))
        return b.fetch(indptr), b.fetch(ids), (b.fetch(sp) if spans else None)


def unigram_ids_utf8_batch(blobs, unigram, unk_id=-1):
    """list[bytes] (UTF-8) -> (indptr, ids, spans) of unigram_ids_utf8_csr, int64 ('' and whitespace-only -> empty rows)"""
    unk_id = _unk32(unk_id)
    _handle_of(Unigram, unigram, "unigram")
    utf8, byte_off = pack_utf8(blobs)
    return unigram_ids_utf8_csr(utf8, byte_off, unigram, unk_id, np.int64, True)


def unigram_ids_batch(texts, unigram, unk_id=-1):
    """list[str] -> (indptr, ids, spans): unigram_ids_utf8_batch of the strings' UTF-8 ("surrogatepass"); the spans are in bytes"""
    return unigram_ids_utf8_batch([t.encode("utf-8", "surrogatepass") for t in texts], unigram, unk_id)


def unigram_encode_utf8_batch(blobs, unigram, max_length, bos_id=None, eos_id=None, pad_id=0, unk_id=-1):
    """list[bytes] (UTF-8) -> (input_ids int32[n, max_length], attention_mask int32[n, max_length]).  Row s = ``bos_id``, the first
    pieces of string s, ``eos_id``, then ``pad_id``; the two specials are added when BOTH are given and omitted when both are None.  A
    longer row is truncated to ``max_length`` cells, specials included.  attention_mask is 1 on the cells in front of the padding.
    One call of ``latok_unigram_padded_utf8_bytes_batch``."""
    unk_id, pad_id = _unk32(unk_id), _unk32(pad_id)
    if (bos_id is None) != (eos_id is None):
        raise ValueError("bos_id and eos_id go together: give both or neither")
    special = bos_id is not None
    bos_id, eos_id = (_unk32(bos_id), _unk32(eos_id)) if special else (0, 0)
    if not isinstance(max_length, (int, np.integer)) or isinstance(max_length, bool) or not 1 + 2 * special <= int(max_length) <= 0x7FFFFFFF:
        raise ValueError("max_length must be an int >= %d" % (1 + 2 * special))
    handle = _handle_of(Unigram, unigram, "unigram")
    utf8, byte_off = pack_utf8(blobs)
    n_str, max_length = len(blobs), int(max_length)
    with _HostBatch(utf8, byte_off) as b:
        input_ids, lengths = b.out((n_str, max_length), np.int32), b.out(n_str, np.int32, True)
        _lib.check(b.lib.latok_unigram_padded_utf8_bytes_batch(b.u8, b.off, n_str, b.total, handle, unk_id, max_length, 1 if special else 0, bos_id,
                                                               eos_id, pad_id, _arg(input_ids), _arg(lengths), None, b.flags, None))
        input_ids, lengths = b.fetch(input_ids), b.fetch(lengths)
    mask = (np.arange(max_length, dtype=np.int32)[None, :] < lengths[:, None]).astype(np.int32)
    return input_ids, mask


# decoding: ids back to UTF-8 bytes on the device, for the ids of BPE and WordPiece alike
DETOK_MODES = {"concat": 0, "wordpiece": 1}             # LATOK_DETOK_CONCAT / LATOK_DETOK_WORDPIECE


class Detokenizer(_DeviceObject):
    """A decoder on the device of the current context (``latok_detok_create``): ``words`` is a list of ``bytes`` or ``str`` (``str`` is
    encoded as UTF-8 with surrogatepass), ``ids`` an optional int32 per word (default: its index; of several words with one id the
    lowest index wins).  ``mode="concat"``: a row decodes to the concatenation of its words -- ``tiktoken``'s ``decode_bytes``;
    ``prefix`` and ``sep`` are not used.  ``mode="wordpiece"``: the first word of a row verbatim, a later word that starts with
    ``prefix`` (0 .. 8 bytes) and is longer than it without the prefix, any other later word behind the ``sep`` byte -- the
    ``" ".join(tokens).replace(" ##", "")`` rule of BERT tokenizers.  Ids in a call's ``skip_ids`` and ids the object does not hold
    leave no trace.  Bytes out: the caller decodes them.  Immutable; ``len()`` is the number of words given.  Freed by ``close()``,
    on leaving a ``with`` block, or with the object."""

    _destroy, _closed = "latok_detok_destroy", "detok must be an open latok_amd.batch.Detokenizer"

    def __init__(self, words, ids=None, mode="concat", prefix=b"##", sep=b" "):
        if mode not in DETOK_MODES:
            raise ValueError('mode must be "concat" or "wordpiece"')
        wordpiece = mode == "wordpiece"
        prefix = (prefix.encode("utf-8") if isinstance(prefix, str) else bytes(prefix)) if wordpiece else b""
        if len(prefix) > 8:
            raise ValueError("prefix must be 0 .. 8 bytes")
        sep = _sep_byte(sep.encode("utf-8") if isinstance(sep, str) else sep) if wordpiece else 0
        data, off, ids = _pack_words(words, ids)
        lib = _lib.ensure_init()
        h = C.c_void_p()
        pre = np.frombuffer(prefix + b"\x00", np.uint8)
        _lib.check(lib.latok_detok_create(_ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(ids) if ids is not None else None,
                                          DETOK_MODES[mode], _ptr(pre), len(prefix), sep, C.byref(h)))
        self._lib, self.handle, self._n = lib, h, off.size - 1
        self.mode, self.prefix, self.sep = mode, prefix, bytes([sep]) if wordpiece else b""

    @classmethod
    def from_tiktoken_file(cls, path):
        """the decoder of a ``.tiktoken`` file (what ``BPE.from_tiktoken_file`` reads): id = rank, ``mode="concat"``"""
        import base64
        with open(path, "rb") as f:
            pairs = [line.split() for line in f.read().splitlines() if line.strip()]
        try:
            words, ids = [base64.b64decode(p[0], validate=True) for p in pairs], [int(p[1]) for p in pairs]
            if any(len(p) != 2 for p in pairs):
                raise ValueError
        except Exception:
            raise ValueError("a line of a .tiktoken file is `base64(token) rank`") from None
        return cls(words, ids or None)

    @classmethod
    def from_vocab_file(cls, path, prefix=b"##", sep=b" "):
        """the decoder of a BERT ``vocab.txt`` (what ``WordPiece.from_vocab_file`` reads): id = line number, ``mode="wordpiece"``"""
        with open(path, "rb") as f:
            words = [line.rstrip(b"\r\n") for line in f.read().split(b"\n")]
        if words and words[-1] == b"":
            words.pop()
        return cls(words, mode="wordpiece", prefix=prefix, sep=sep)

    def info(self):
        """dict of what ``latok_detok_info`` reports"""
        v = [C.c_int64(0) for _ in range(4)]
        mode, dense, dev = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._lib.latok_detok_info(self._open(), *[C.byref(x) for x in v], C.byref(mode), C.byref(dense), C.byref(dev)))
        return dict(n_words=v[0].value, n_ids=v[1].value, blob_bytes=v[2].value, max_len=v[3].value, mode=mode.value, dense=dense.value,
                    device=dev.value)

    def __len__(self):
        return self._n


def _decode(detok, skip_ids, errors, n_rows, entry):
    """the size query, then the fill of one decode call -> (out_bytes, out_off); ``entry(lib, handle, skip, n_skip, out, cap, out_off, n, unk)``"""
    if errors not in ("strict", "ignore"):
        raise ValueError('errors must be "strict" or "ignore"')
    skip = list(skip_ids)
    if len(skip) > 16:
        raise ValueError("skip_ids holds at most 16 ids")
    skip = _int32_each(skip, len(skip), "skip_ids", "skipped id")
    handle = _handle_of(Detokenizer, detok, "detok")
    lib = _lib.ensure_init()
    out_off, n, unk = np.zeros(n_rows + 1, np.int64), C.c_int64(0), C.c_int64(0)

    def call(out=None, cap=0):
        return entry(lib, handle, _ptr(skip) if skip.size else None, skip.size, out, cap, _ptr(out_off), C.byref(n), C.byref(unk))

    _, (out,) = _size_then_fill(call, n, lambda k: (np.empty(k, np.uint8),))
    if errors == "strict" and unk.value:
        raise ValueError("%d ids are not in the decoder (errors=\"ignore\" drops them)" % unk.value)
    return out, out_off


def decode_csr(detok, indptr, ids, skip_ids=(), errors="strict"):
    """(out_bytes uint8[], out_off int64[n + 1]): row s of the CSR (``indptr`` int32 or int64, ``ids`` int32) decoded by ``detok``;
    row s = out_bytes[out_off[s]:out_off[s+1]].  Ids in ``skip_ids`` (at most 16: pad / BOS / EOS / [CLS] / [SEP]) and unknown ids
    leave no trace; ``errors="strict"`` raises ValueError naming the count when any id was unknown, ``"ignore"`` returns the bytes.
    Decoded on the device (``latok_detok_csr``): the size query, then the fill."""
    ids = np.asarray(ids)
    ids = _int32_each(ids, ids.size if ids.ndim == 1 else -1, "ids", "piece")
    indptr, ids, flags = _csr_arrays(indptr, ids)
    return _decode(detok, skip_ids, errors, indptr.size - 1,
                   lambda lib, h, skip, n_skip, out, cap, out_off, n, unk: lib.latok_detok_csr(
                       h, _ptr(indptr), _ptr(ids) if ids.size else None, indptr.size - 1, ids.size, skip, n_skip, out, cap, out_off, n, unk, flags, None))


def decode_padded(detok, input_ids, lengths=None, attention_mask=None, skip_ids=(), errors="strict"):
    """(out_bytes, out_off) of decode_csr for the padded ``input_ids`` int32[n, max_length] of the ``*_encode_utf8_batch`` calls: row s
    is its first ``lengths[s]`` cells; ``attention_mask`` (its row sums are the lengths) may be given instead; with neither, every
    cell counts and the pad id belongs into ``skip_ids``.  One call of ``latok_detok_padded`` per pass."""
    block = np.asarray(input_ids)
    if block.ndim != 2 or (block.size and block.dtype.kind not in "iu"):
        raise ValueError("input_ids must be a 2-d integer array [n, max_length]")
    n_rows, max_length = block.shape
    block = _int32_each(block.reshape(-1), block.size, "input_ids", "cell")
    if lengths is not None and attention_mask is not None:
        raise ValueError("give lengths or attention_mask, not both")
    if attention_mask is not None:
        mask = np.asarray(attention_mask)
        if mask.shape != (n_rows, max_length):
            raise ValueError("attention_mask must have the shape of input_ids")
        lengths = (mask != 0).sum(axis=1)
    if lengths is not None:
        lengths = _int32_each(lengths, n_rows, "lengths", "row")
    return _decode(detok, skip_ids, errors, n_rows,
                   lambda lib, h, skip, n_skip, out, cap, out_off, n, unk: lib.latok_detok_padded(
                       h, _ptr(block) if block.size else None, _ptr(lengths) if lengths is not None and n_rows else None, n_rows, max_length, skip,
                       n_skip, out, cap, out_off, n, unk, 0, None))


def decode_batch(detok, rows, skip_ids=(), errors="strict"):
    """list[bytes]: the decoded rows.  ``rows`` is a list of int sequences (decode_csr) or a 2-d int32 array (decode_padded with every
    cell counted: put the pad id into ``skip_ids``)."""
    if isinstance(rows, np.ndarray) and rows.ndim == 2:
        out, off = decode_padded(detok, rows, skip_ids=skip_ids, errors=errors)
    else:
        rows = [np.asarray(r).reshape(-1) if len(r) else np.zeros(0, np.int32) for r in rows]   # (an empty list has no integer dtype of its own)
        indptr = np.zeros(len(rows) + 1, np.int64)
        np.cumsum([r.size for r in rows], out=indptr[1:])
        ids = np.concatenate(rows) if rows and indptr[-1] else np.zeros(0, np.int32)
        out, off = decode_csr(detok, indptr, ids, skip_ids, errors)
    data = out.tobytes()
    return [data[off[s]:off[s + 1]] for s in range(off.size - 1)]


# token counts: the vocabulary of a corpus -- every distinct token with its frequency --, counted on the device, exactly
class TokenCounter(_DeviceObject):
    """A counting table on the device of the current context (``latok_counter_create``): at most about ``max_words`` distinct
    tokens (the table has ``n_slots`` >= 2 * max_words slots), each of at most ``max_word_bytes`` bytes (1 .. 256; longer tokens
    are tallied as ``long``), placed by MurmurHash3 with ``seed``.  ``update*`` count the tokens of a batch -- the byte slices
    token_spans_utf8_bytes_csr reports -- and return that call's ``{tokens, counted, long, dropped}``; ``stats`` are the totals
    with ``distinct``.  ``dropped == 0`` means every count is exact.  Mutable, so it has no flow form.  Freed by ``close()``, on
    leaving a ``with`` block, or with the object."""

    STATS = ("tokens", "counted", "long", "dropped", "distinct")
    _destroy, _closed = "latok_counter_destroy", "the TokenCounter is closed"

    def __init__(self, max_words, max_word_bytes=256, seed=0):
        seed = _seed32(seed)
        for name, v, hi in (("max_words", max_words, 1 << 30), ("max_word_bytes", max_word_bytes, 256)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= int(v) <= hi:
                raise ValueError("%s must be an int in 1 .. %d" % (name, hi))
        lib = _lib.ensure_init()
        h = C.c_void_p()
        _lib.check(lib.latok_counter_create(int(max_words), int(max_word_bytes), seed, C.byref(h)))
        self._lib, self.handle, self.seed = lib, h, seed
        self.max_words, self.max_word_bytes = int(max_words), int(max_word_bytes)
        n_slots = C.c_int64(0)
        _lib.check(lib.latok_counter_info(h, None, C.byref(n_slots), None, None, None, None))
        self.n_slots = n_slots.value

    def update_utf8_csr(self, utf8, byte_off):
        """count the tokens of a CSR batch of UTF-8 bytes; returns this call's {tokens, counted, long, dropped}"""
        utf8, byte_off = _csr_u8(utf8, byte_off)
        h = self._open()
        n_str = byte_off.size - 1
        total = int(byte_off[-1]) if n_str > 0 else 0
        st = np.zeros(4, np.int64)
        _lib.check(self._lib.latok_count_tokens_utf8_bytes_batch(_ptr(utf8), _ptr(byte_off), n_str, total, h, _ptr(st), 0, None))
        return dict(zip(self.STATS[:4], map(int, st)))

    def update_utf8(self, blobs):
        """list[bytes] (UTF-8)"""
        self._open()
        return self.update_utf8_csr(*pack_utf8(blobs))

    def update(self, texts):
        """list[str]; the strings go through UTF-8 ("surrogatepass") on the host"""
        return self.update_utf8([t.encode("utf-8", "surrogatepass") for t in texts])

    @property
    def stats(self):
        h = self._open()
        st = np.zeros(5, np.int64)
        _lib.check(self._lib.latok_counter_info(h, None, None, None, None, None, _ptr(st)))
        return dict(zip(self.STATS, map(int, st)))

    def items(self):
        """(list[bytes], uint64 array): the words held and their counts, in no particular order.  One state of the counter: when another
        thread's update lands between the size query and the read, the read reports the larger need and is made again with it (which
        is why this is not _size_then_fill: there a refused fill is an error)."""
        h = self._open()
        n, nb = C.c_int64(0), C.c_int64(0)
        rc = self._lib.latok_counter_read(h, None, 0, None, None, 0, C.byref(n), C.byref(nb))   # the size query
        while True:
            if rc != _lib.OK and not (rc == _lib.ERR_INVALID and n.value > 0):
                _lib.check(rc)
            if n.value == 0:
                return [], np.zeros(0, np.uint64)
            cap, bytes_cap = n.value, nb.value
            words, off, counts = np.empty(bytes_cap, np.uint8), np.empty(cap + 1, np.int64), np.empty(cap, np.uint64)
            rc = self._lib.latok_counter_read(h, _ptr(words), bytes_cap, _ptr(off), _ptr(counts), cap, C.byref(n), C.byref(nb))
            if rc == _lib.ERR_INVALID and (n.value > cap or nb.value > bytes_cap):
                continue                                      # the counter grew in between: again, with the sizes this read reported
            _lib.check(rc)
            raw = words.tobytes()
            return [raw[off[i]:off[i + 1]] for i in range(n.value)], counts[:n.value].copy()

    def most_common(self, n=None):
        """[(word bytes, count)] sorted by (-count, bytes): deterministic; the first ``n`` if given"""
        words, counts = self.items()
        ranked = sorted(zip(words, map(int, counts)), key=lambda wc: (-wc[1], wc[0]))
        return ranked if n is None else ranked[:n]

    def to_vocab(self, min_count=1, max_size=None, seed=0):
        """a ``Vocab`` of the words counted at least ``min_count`` times, at most ``max_size`` of them; a word's id is its rank
        in ``most_common()``"""
        seed = _seed32(seed)
        return Vocab([w for w, c in self.most_common(max_size) if c >= min_count], seed=seed)

    def clear(self):
        h = self._open()
        _lib.check(self._lib.latok_counter_clear(h))


def count_tokens_utf8_batch(blobs, max_words=None):
    """list[bytes] (UTF-8) -> ``collections.Counter`` of the batch's tokens (as bytes), counted on the device.  ``max_words``
    defaults to the byte total (at most 2**30): a token has at least one byte, so the table is at most half full and does not
    drop in practice (a drop needs 128 occupied slots in a row, about 1e-11 per slot at that load).  That default is sized for
    the worst case, not for text: it costs 32 bytes of device memory per input byte, rounded up to a power of two (4 GiB for a
    100 MB batch) -- pass ``max_words`` (about the number of distinct tokens expected) for anything large, or keep a
    ``TokenCounter`` and check ``stats["dropped"]``.  A ``dropped`` count other than 0 raises ``RuntimeError`` here, since
    the Counter would not be exact.  Tokens of more than 256 bytes are not counted."""
    import collections
    total = sum(len(b) for b in blobs)
    if max_words is None:
        max_words = min(max(total, 1), 1 << 30)
    with TokenCounter(max_words) as tc:
        if total and tc.update_utf8(blobs)["dropped"]:
            raise RuntimeError("count_tokens_utf8_batch: max_words=%d is too small for this batch, tokens were dropped" % max_words)
        words, counts = tc.items()
    return collections.Counter(dict(zip(words, map(int, counts))))


# ---- PEP 393 code units: 1 / 2 / 4 bytes per char, the buffer the reference itself reads (latok.c:53-55,79) -----------
def pack_kind(texts):
    """list[str] -> (units, row_off): units uint8 / uint16 / uint32 = the narrowest PEP 393 kind that holds every char of
    the batch (what CPython stores for the joined text), row_off int64[n+1] in chars."""
    lens = np.fromiter((len(t) for t in texts), dtype=np.int64, count=len(texts))
    row_off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum(lens, out=row_off[1:])
    joined = "".join(texts)
    try:
        units = np.frombuffer(joined.encode("latin-1"), dtype=np.uint8)
    except UnicodeEncodeError:
        blob = joined.encode("utf-16-le", "surrogatepass")
        if len(blob) == 2 * len(joined):
            units = np.frombuffer(blob, dtype="<u2").astype(np.uint16, copy=False)
        else:   # astral chars: kind 4
            units = np.frombuffer(joined.encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.uint32, copy=False)
    return np.ascontiguousarray(units), row_off


def _csr_kind(units, row_off):
    units = np.ascontiguousarray(units)
    if units.dtype not in (np.uint8, np.uint16, np.uint32):
        raise ValueError("units must be uint8 (Latin-1), uint16 (UCS-2) or uint32 (UCS-4)")
    row_off = np.ascontiguousarray(row_off, dtype=np.int64)
    if row_off.ndim != 1 or row_off.size < 1:
        raise ValueError("row_off must be a 1-D array of n_str + 1 offsets")
    if units.ndim != 1 or (row_off.size > 1 and units.size < int(row_off[-1])):
        raise ValueError("units is shorter than row_off[-1]")
    return units, row_off, int(units.dtype.itemsize)


def split_mask_kind_csr(units, row_off) -> np.ndarray:
    """split_mask_batch for PEP 393 code units (dtype picks the kind); bit i = packed char i starts a token."""
    units, row_off, kind = _csr_kind(units, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    bits = np.zeros((total + 63) // 64, np.uint64)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_split_mask_kind_batch(_ptr(units), kind, _ptr(row_off), n_str, total, _ptr(bits), 0, None))
    return bits


def _compact_kind(fn, width, units, row_off, dtype, feats=False):
    units, row_off, kind = _csr_kind(units, row_off)
    n_str = row_off.size - 1
    total = int(row_off[-1]) if n_str > 0 else 0
    return _compact(fn, [_ptr(units), kind, _ptr(row_off)], n_str, total, width, dtype, feats)


def split_offsets_kind_csr(units, row_off, dtype=np.int64):
    """(counts, offsets) like split_offsets_csr for PEP 393 code units."""
    return _compact_kind(_lib.ensure_init().latok_split_offsets_kind_batch, 1, units, row_off, dtype)


def token_spans_kind_csr(units, row_off, dtype=np.int64):
    """(counts, spans[n_tokens, 2]) like token_spans_csr for PEP 393 code units."""
    return _compact_kind(_lib.ensure_init().latok_token_spans_kind_batch, 2, units, row_off, dtype)


def token_features_kind_csr(units, row_off, dtype=np.int64):
    """(counts, spans[n_tokens, 4], features int8[n_tokens, 25]) like token_features_csr for PEP 393 code units."""
    return _compact_kind(_lib.ensure_init().latok_token_features_kind_batch, 4, units, row_off, dtype, feats=True)


def spans_from_offsets(text, nz):
    """Token strings of one text from its boundary offsets, as the reference's loop builds them
    (default_tokenizer.py:149-158): slice between consecutive boundaries, strip, drop empties."""
    toks = []
    if len(nz) > 0:
        bounds = [int(x) for x in nz]
        a, end = bounds[0], 0
        for end in bounds[1:]:
            tok = text[a:end].strip()
            if tok:
                toks.append(tok)
            a = end
        tok = text[end:].strip()
        if tok:
            toks.append(tok)
    return toks


def tokenize_batch(texts, devices=None):
    """list[str] -> list[list[str]], each as list(tokenize(text)) of the reference (default_tokenizer.py:137-160);
    an empty string yields [] instead of the reference's IndexError.
    devices: a multi.DevicePool or a list of device ids -> the strings are sharded over them, one host thread and one
    library context per entry (latok_amd.multi); the result is the same list."""
    if len(texts) == 0:
        return []
    if devices is not None:
        from . import multi
        return multi.tokenize_batch(texts, devices)
    if _narrow_pays(texts):
        units, row_off = pack_kind(texts)
        counts, spans = token_spans_kind_csr(units, row_off, dtype=_record_dtype(row_off))
    else:
        cps, row_off = pack(texts)
        counts, spans = token_spans_csr(cps, row_off, dtype=_record_dtype(row_off))
    out, k = [], 0
    for text, n in zip(texts, counts.tolist()):
        out.append([text[a:b] for a, b in spans[k:k + n].tolist()])
        k += n
    return out


class TokenSpans:
    """The tokens of a batch WITHOUT the per-token Python objects: ``spans[k] = (start, end)`` of token k inside its own
    string (whitespace stripped, empties dropped -- what the reference's loop keeps, default_tokenizer.py:149-160),
    ``counts[i]`` tokens for string i, strings in order.  Building ``list[list[str]]`` costs one slice per token (1.5 ms per
    1000 short strings, five orders of magnitude below the device path); a caller that filters, counts, hashes or looks only
    at some strings slices lazily:

        ts = batch.token_spans_batch(texts)
        ts.counts, ts.spans                     # numpy: int32 / int64 [n_str], [n_tokens, 2]
        ts.tokens(i)                            # list[str] of string i, sliced on demand
        for toks in ts: ...                     # == batch.tokenize_batch(texts), one string at a time
    """

    def __init__(self, texts, counts, spans):
        self.texts, self.counts, self.spans = texts, counts, spans
        self.first = np.zeros(len(texts) + 1, np.int64)       # index of each string's first token
        np.cumsum(counts, out=self.first[1:])

    def __len__(self):
        return len(self.texts)

    def row(self, i):
        """(start, end) pairs of string i: a view into ``spans``"""
        return self.spans[int(self.first[i]):int(self.first[i + 1])]

    def tokens(self, i):
        t = self.texts[i]
        return [t[a:b] for a, b in self.row(i).tolist()]

    def __iter__(self):
        return (self.tokens(i) for i in range(len(self.texts)))


def token_spans_batch(texts):
    """list[str] -> TokenSpans: the same device work as tokenize_batch, none of its per-token Python."""
    texts = list(texts)
    if len(texts) == 0:
        return TokenSpans(texts, np.zeros(0, np.int64), np.zeros((0, 2), np.int64))
    if _narrow_pays(texts):
        units, row_off = pack_kind(texts)
        counts, spans = token_spans_kind_csr(units, row_off, dtype=_record_dtype(row_off))
    else:
        cps, row_off = pack(texts)
        counts, spans = token_spans_csr(cps, row_off, dtype=_record_dtype(row_off))
    return TokenSpans(texts, counts, spans.reshape(-1, 2))


# ---- runtime rule tables (the reference's extension point, default_tokenizer.py:9-30,108-110) ------------------------
# ---- batch flow: many device-resident batches through the current context, two in flight ------------------------------
def flow_split_mask(d_cps, d_row_off, n_str, total_chars, d_mask):
    """include/latok_hip.h "batch flow": enqueue the split mask of one DEVICE-RESIDENT batch (device addresses as ints /
    c_void_p: UTF-32 code points, int64 row offsets, uint64 mask words out) and return at once; up to two batches run
    overlapped (the string-index and resolve launches of one in the shadow of the other's tile kernel).  The inputs must
    be complete in device memory; results are complete after ``flow_wait()``.  The reference's unit of independence is
    the single ``tokenize`` call (default_tokenizer.py:137-160)."""
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_split_mask(d_cps, d_row_off, int(n_str), int(total_chars), d_mask))


def flow_split_mask_kind(d_units, kind, d_row_off, n_str, total_chars, d_mask):
    """``flow_split_mask`` for PEP 393 units in device memory (kind 1 = Latin-1 bytes, 2 = UCS-2 uint16, 4 = UTF-32)."""
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_split_mask_kind(d_units, int(kind), d_row_off, int(n_str), int(total_chars), d_mask))


def flow_split_mask_utf8_bytes(d_utf8, d_byte_off, n_str, total_bytes, d_mask):
    """``flow_split_mask`` in byte space: UTF-8 bytes + byte offsets in device memory, bit i of the mask = byte i."""
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_split_mask_utf8_bytes(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_mask))


def flow_split_offsets(d_units, kind, d_row_off, n_str, total_units, d_counts, d_offsets, cap, d_result, dtype=np.int64):
    """Boundary offsets of one device-resident batch through the flow (``latok_flow_split_offsets``): kind 4 / 1 / 2 =
    UTF-32 / Latin-1 / UCS-2 units, 0 = UTF-8 bytes in byte space.  ``d_result`` = int64[2] the device can write: item
    total and error word, valid after ``flow_wait()``; nothing is written to ``d_offsets`` when the total exceeds ``cap``."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_split_offsets(d_units, int(kind), d_row_off, int(n_str), int(total_units), d_counts, d_offsets, int(cap),
                                            d_result, flag32))


def flow_token_spans(d_units, kind, d_row_off, n_str, total_units, d_counts, d_spans, cap, d_result, dtype=np.int64):
    """Token spans (start, end per kept token) of one device-resident batch through the flow (``latok_flow_token_spans``)."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_token_spans(d_units, int(kind), d_row_off, int(n_str), int(total_units), d_counts, d_spans, int(cap),
                                          d_result, flag32))


def flow_token_features(d_units, kind, d_row_off, n_str, total_chars, d_counts, d_spans4, d_features, cap, d_result, dtype=np.int64):
    """featurize of one device-resident batch through the flow (``latok_flow_token_features``): 4 span values + 25 int8
    feature sums per kept token (reference default_tokenizer.py:163-191)."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_token_features(d_units, int(kind), d_row_off, int(n_str), int(total_chars), d_counts, d_spans4, d_features,
                                             int(cap), d_result, flag32))


def flow_split_mask_utf8(d_utf8, d_byte_off, n_str, total_bytes, d_mask, mask_cap_words, d_cp_row_off, d_result):
    """Split mask of one device-resident UTF-8 batch in CODE-POINT units through the flow (``latok_flow_split_mask_utf8``):
    what ``split_mask_utf8_batch`` reports (bit k = code point k, the reference's unit, latok.c:53-55,79) without a wait.
    ``d_result`` = int64[4] the device can write, valid after ``flow_wait()``: [0] 0, [1] error word, [2] code-point total,
    [3] nonzero = malformed UTF-8 -- nothing of the batch is valid, resubmit it through the blocking call."""
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_split_mask_utf8(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_mask, int(mask_cap_words),
                                              d_cp_row_off, d_result))


def flow_split_offsets_utf8(d_utf8, d_byte_off, n_str, total_bytes, d_counts, d_offsets, cap, d_result, dtype=np.int64):
    """Boundary offsets in code-point units of one device-resident UTF-8 batch through the flow
    (``latok_flow_split_offsets_utf8``).  ``d_result`` = int64[4]: item total, error word, code-point total, malformed flag."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_split_offsets_utf8(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_counts, d_offsets, int(cap),
                                                 d_result, flag32))


def flow_token_spans_utf8(d_utf8, d_byte_off, n_str, total_bytes, d_counts, d_spans, cap, d_result, dtype=np.int64):
    """Token spans in code-point units of one device-resident UTF-8 batch through the flow (``latok_flow_token_spans_utf8``)."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_token_spans_utf8(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_counts, d_spans, int(cap),
                                               d_result, flag32))


def flow_token_features_utf8(d_utf8, d_byte_off, n_str, total_bytes, d_counts, d_spans4, d_features, cap, d_result, dtype=np.int64):
    """featurize in code-point units of one device-resident UTF-8 batch through the flow (``latok_flow_token_features_utf8``)."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_token_features_utf8(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_counts, d_spans4, d_features,
                                                  int(cap), d_result, flag32))


def flow_token_features_utf8_bytes(d_utf8, d_byte_off, n_str, total_bytes, d_counts, d_spans4, d_features, cap, d_result, dtype=np.int64):
    """featurize in BYTE space of one device-resident UTF-8 batch through the flow (``latok_flow_token_features_utf8_bytes``):
    span records in byte positions, sums per char.  ``d_result`` = int64[4]: token total, error word, code-point total,
    malformed flag (nonzero: no record and no sum of the batch was written)."""
    lib = _lib.ensure_init()
    _, flag32 = _out_dtype(dtype)
    _lib.check(lib.latok_flow_token_features_utf8_bytes(d_utf8, d_byte_off, int(n_str), int(total_bytes), d_counts, d_spans4, d_features,
                                                        int(cap), d_result, flag32))


def flow_join_tokens_utf8_bytes(d_utf8, d_byte_off, n_str, total_bytes, d_out_bytes, out_cap, d_out_off, d_counts, d_result, sep=b" ",
                                dtype=np.int64):
    """joined token text of one device-resident UTF-8 batch through the flow (``latok_flow_join_tokens_utf8_bytes``): what
    ``join_tokens_utf8_csr`` reports, in device buffers, without waiting.  ``d_result`` = int64[2]: output bytes, error word
    (bit 2: the batch needs more than ``out_cap`` bytes and nothing was written to ``d_out_bytes``); ``d_counts`` may be None.
    The arguments follow the C call, except that ``sep`` (its fifth) is a trailing keyword here and ``flags`` is ``dtype`` (the
    width of the counts), as in the sibling wrappers."""
    sep = _sep_byte(sep)
    _, flag32 = _out_dtype(dtype)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_join_tokens_utf8_bytes(d_utf8, d_byte_off, int(n_str), int(total_bytes), sep, d_out_bytes, int(out_cap),
                                                     d_out_off, d_counts, d_result, flag32))


def flow_token_hashes_utf8_bytes(d_utf8, d_byte_off, n_str, total_bytes, d_counts, d_spans, d_hashes, cap, d_result, seed=0,
                                 dtype=np.int64):
    """token hashes of one device-resident UTF-8 batch through the flow (``latok_flow_token_hashes_utf8_bytes``): what
    ``token_hashes_utf8_csr`` reports, in device buffers, without waiting.  ``d_result`` = int64[2]: tokens, error word; more
    tokens than ``cap`` means nothing was written to ``d_hashes`` / ``d_spans``.  ``d_counts`` and ``d_spans`` may be None.  The
    arguments follow the C call, except that ``seed`` (its fifth) is a trailing keyword here and ``flags`` is ``dtype`` (the width
    of counts and spans), as in the sibling wrappers."""
    seed = _seed32(seed)
    _, flag32 = _out_dtype(dtype)
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_token_hashes_utf8_bytes(d_utf8, d_byte_off, int(n_str), int(total_bytes), seed, d_counts, d_spans, d_hashes,
                                                      int(cap), d_result, flag32))


def flow_token_ids_utf8_bytes(d_utf8, d_byte_off, n_str, total_bytes, vocab, d_counts, d_spans, d_ids, cap, d_result, unk_id=-1,
                              dtype=np.int64):
    """token ids of one device-resident UTF-8 batch through the flow (``latok_flow_token_ids_utf8_bytes``): what
    ``token_ids_utf8_csr`` reports, in device buffers, without waiting.  ``d_result`` = int64[2]: tokens, error word; more tokens
    than ``cap`` means nothing was written to ``d_ids`` / ``d_spans``.  ``d_counts`` and ``d_spans`` may be None.  The arguments
    follow the C call, except that ``unk_id`` is a trailing keyword here and ``flags`` is ``dtype`` (the width of counts and
    spans), as in the sibling wrappers."""
    unk_id = _unk32(unk_id)
    _, flag32 = _out_dtype(dtype)
    handle = _handle_of(Vocab, vocab, "vocab")
    lib = _lib.ensure_init()
    _lib.check(lib.latok_flow_token_ids_utf8_bytes(d_utf8, d_byte_off, int(n_str), int(total_bytes), handle, unk_id, d_counts, d_spans, d_ids,
                                                   int(cap), d_result, flag32))


def flow_wait():
    """Block until every batch submitted with ``flow_split_mask`` on the current context is complete."""
    _lib.check(_lib.ensure_init().latok_flow_wait())


def _rule_table(name, idx):
    """A combo matrix as build_combo_matrix returns it -> C-contiguous int8 [rows, cols].  A 1-D index vector means
    "sum of those feature rows" to _combine_matrix_rows (latok.c:340-353): one single-column row per entry."""
    a = np.asarray(idx)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: feature ids must be integers")
    if a.size and not ((a == -1) | ((a >= 0) & (a < _lib.FEATURE_COUNT))).all():
        raise ValueError(f"{name}: feature ids must be -1 (padding) or 0..{_lib.FEATURE_COUNT - 1}")
    a = a.astype(np.int8)
    if a.ndim == 1:
        a = a[a != -1].reshape(-1, 1)
    if a.ndim != 2:
        raise ValueError(f"{name}: must be a 1-D or 2-D index matrix")
    if a.shape[0] and a.shape[1] == 0:
        raise ValueError(f"{name}: rows have no columns")
    return np.ascontiguousarray(a)


def set_rules(c_split, c_mask, c_sym):
    """Install custom C_SPLIT / C_MASK / C_SYM combo matrices: every batch entry point (and ``tokenize`` / ``featurize``
    of latok_amd.core.default_tokenizer) then evaluates them inside the fused kernel, bit-exact with the reference's
    ``gen_split_mask`` recipe (default_tokenizer.py:113-134) run on the same tables.  ``reset_rules()`` restores the
    built-in tables."""
    lib = _lib.ensure_init()
    t = [_rule_table(n, m) for n, m in (("C_SPLIT", c_split), ("C_MASK", c_mask), ("C_SYM", c_sym))]
    args = []
    for a in t:
        args += [_ptr(a) if a.size else None, a.shape[0], a.shape[1] if a.shape[0] else 0]
    _lib.check(lib.latok_set_rules(*args))


def reset_rules():
    _lib.check(_lib.ensure_init().latok_reset_rules())


def rules_active() -> bool:
    return bool(_lib.ensure_init().latok_rules_active())
