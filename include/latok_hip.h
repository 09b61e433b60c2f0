/* latok_hip.h -- C ABI of liblatok_hip.so: latok's character-feature-matrix + split-mask path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference binds this path through the CPython extension module `latok.latok`
 * (reference setup.py:10-18, method table latok/core/src/latok/latok.c:373-378) whose three functions are called by
 * latok/core/default_tokenizer.py:36,123-129,146 and latok/core/latok_utils.py:7,15,24.  Each entry point below names
 * the reference interface it replaces.  Plain pointers and sizes only: no Python.h, no NumPy C-API, no torch types.
 *
 * Conventions
 *   - every function returns LATOK_OK (0) or a negative LATOK_ERR_*; latok_last_error() gives the message
 *     (the reference raises ValueError for bad arguments: latok.c:40-50,151-171,292-312; the Python mirror maps
 *     LATOK_ERR_INVALID -> ValueError and everything else -> RuntimeError).
 *   - the caller owns every buffer (the reference returns freshly allocated NumPy arrays: latok.c:59,174,357).
 *   - `flags & LATOK_DEVICE_PTRS`: all data pointers are device pointers, the call is asynchronous on `stream`
 *     (a hipStream_t, NULL = the library's own stream) and returns as soon as the work is enqueued.  Otherwise they
 *     are host pointers: the library stages through its own device buffers and the call is synchronous.
 *   - a batch is CSR: `cps` = packed UTF-32 code points of all strings, `row_off[n_str + 1]` = start of each string
 *     (row_off[0] == 0, non-decreasing).  Device `cps` pointers must be 16-byte aligned.  Host-pointer calls check
 *     row_off and fail with LATOK_ERR_INVALID; device-resident row offsets cannot be checked without a copy, so a caller
 *     that passes device pointers guarantees them (results are undefined otherwise).
 *   - `total_chars` = row_off[n_str]; the caller normally knows it.  Pass -1 to let the library read it (in device
 *     mode that costs one blocking 8-byte device->host copy).
 *   - contexts, threads and streams: every entry point works on the calling thread's CURRENT CONTEXT (see "contexts"
 *     below; default = the process-wide one latok_init creates).  A context owns one device, one stream, one set of
 *     device workspaces and one lock: calls on the same context are serialised and ordered on the device (a call waits
 *     for the previous call's last kernel before its own first one, whatever stream it uses); calls on DIFFERENT
 *     contexts share nothing and run concurrently -- one host thread + one context per GPU is how a batch is sharded
 *     over the GPUs of a node (SURVEY 8b "Threading", 8e).  The compaction entry points (offsets / spans / features)
 *     return the item total to the host and therefore block even in device mode: everything is enqueued first (the
 *     kernels write the records only if the total fits the caller's capacity) and the call synchronises once.
 *   - small host batches (host pointers, at most LATOK_TILE_CHARS chars and 512 strings -- one string per call is the
 *     reference's own calling pattern, default_tokenizer.py:137-191) are one single-wavefront launch for offsets, spans
 *     and features alike: inputs and outputs pass through pinned memory the kernel reads / writes directly, and the
 *     call returns when it has seen the completion word the kernel stores after its last output (LATOK_SMALL_POLL=0 in
 *     the environment: wait for the stream instead).  Host batches up to 256 K chars / 16 K strings take the same pinned
 *     route with a handful of launches (up to 24 tiles: one launch for the whole mask pipeline; LATOK_ONE_SEGMENT=0: three).
 *     Small host batches of PEP 393 kind 1 / 2 units are widened, and small well-formed UTF-8 batches decoded, by the host
 *     on their way into that pinned area (byte-space results are mapped back to byte positions), so one string per call
 *     costs the same whatever form it arrives in; malformed UTF-8 and larger batches are read by the device as they are.
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails with LATOK_ERR_HIP.
 */
#ifndef LATOK_HIP_H
#define LATOK_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LATOK_OK 0
#define LATOK_ERR_INVALID (-1)  /* bad argument / shape (reference: ValueError) */
#define LATOK_ERR_HIP (-2)      /* HIP runtime error, or no device */
#define LATOK_ERR_NOT_INIT (-3) /* latok_init() has not been called */
#define LATOK_ERR_NOMEM (-4)

#define LATOK_DEVICE_PTRS 1
/* Compaction entry points (offsets / spans / features): counts_out and the offsets / spans / spans4 records are int32
 * arrays instead of int64 (the parameters keep their int64_t* type: pass the int32 buffer through a cast; capacities stay
 * in ELEMENTS / tokens).  The records are most of the bytes these calls write and send over the bus -- 8 B per boundary,
 * 16 B per token -- so the 32-bit form halves that.  Every value is relative to its own string, so it fits unless a
 * single string has 2^31 chars or more: then the call fails with LATOK_ERR_INVALID and the 64-bit form has to be used. */
#define LATOK_OUT_INT32 2

#define LATOK_FEATURE_COUNT 25 /* reference latok/core/offsets.py:49 */
#define LATOK_TILE_CHARS 4096  /* chars per wavefront tile (64 lanes x 64-bit words) */

/* ---- lifecycle ------------------------------------------------------------------------------------------------ */
int latok_device_count(void);          /* number of HIP devices, 0 when none (never fails) */
int latok_init(int device);            /* create the DEFAULT context on `device`: Unicode tables, stream, workspaces */
int latok_shutdown(void);              /* destroy the default context */
const char* latok_last_error(void);    /* message of the last failure on this thread */
const char* latok_version(void);

/* ---- contexts: one per GPU (or several per GPU) in one process -------------------------------------------------------
 * The reference holds the GIL for a whole call and has no state (latok.c:373-378: three pure functions), so it is
 * re-entrant but never concurrent.  Here the state a call needs (device, stream, tables, workspaces, run-time rule
 * tables) lives in a context.  latok_ctx_create binds a new context to `device`; latok_ctx_set_current makes it the
 * calling THREAD's current context (NULL = back to the default one) -- the model of hipSetDevice -- and every entry point
 * of this header then runs on it: its device, its stream, its rule tables (latok_set_rules is per context).  The
 * caller's current HIP device is never changed by a call.  A context must not be destroyed while another thread still
 * has it current.  Device memory from latok_dev_alloc belongs to the device of the context that was current. */
typedef struct latok_ctx latok_ctx;
int latok_ctx_create(int device, latok_ctx** ctx_out);
int latok_ctx_destroy(latok_ctx* ctx);
int latok_ctx_set_current(latok_ctx* ctx);   /* NULL = the default context */
latok_ctx* latok_ctx_get_current(void);      /* NULL when the thread runs on the default context */
int latok_ctx_device(latok_ctx* ctx);        /* device of a context (NULL = the default one), -1 when not initialised */

/* Grow the library-owned workspace (tile summaries, segment aggregates) for batches of up to
 * `max_chars` code points / `max_strings` strings, so that later calls allocate nothing. */
int latok_reserve(int64_t max_chars, int64_t max_strings);

/* ---- the fused hot path ------------------------------------------------------------------------------------------
 * Replaces, for a whole batch at once, the reference call chain of default_tokenizer.py:146-148:
 *   _gen_parse_matrix (latok.c:31-138) -> gen_split_mask (default_tokenizer.py:113-134: 3x _combine_matrix_rows
 *   latok.c:275-370 + gen_block_mask latok.c:140-258) -> nonzero-ness of the result.
 * mask_bits_out: uint64[ceil(total_chars / 64)], bit (i & 63) of word (i >> 6) = 1 iff packed char i is a token
 * boundary (splits[i] != 0).  Every string's first char is a boundary (default_tokenizer.py:132); empty strings
 * contribute nothing (the reference raises IndexError for '' -- documented deviation of batch mode). */
int latok_split_mask_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                           uint64_t* mask_bits_out, int flags, void* stream);

/* Same pipeline, but writes the reference's split VALUES (0..5, the int8 vector returned by gen_split_mask,
 * default_tokenizer.py:121-134) as uint8[total_chars].  Parity/debug form: 1 byte per char instead of 1 bit. */
int latok_split_values_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                             uint8_t* values_out, int flags, void* stream);

/* Boundary offsets (replaces np.nonzero(splits)[0], default_tokenizer.py:148) for every string of the batch:
 * counts_out[n_str] = number of boundaries of each string; offsets_out[0..sum(counts)) = the offsets of string 0,
 * then string 1, ... each relative to its own string start (int64, ascending, first one always 0).
 * offsets_cap = capacity of offsets_out in elements; *n_offsets_out = total number written (host pointer, always).
 * Returns LATOK_ERR_INVALID if offsets_cap is too small (n_offsets_out still holds the needed size).
 * Synchronous in both pointer modes (the total is returned to the host). */
int latok_split_offsets_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                              int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap, int64_t* n_offsets_out,
                              int flags, void* stream);

/* Token spans: everything tokenize() does after np.nonzero (reference default_tokenizer.py:149-158), on the device:
 * consecutive boundaries delimit a token, leading/trailing SPACE-class chars are stripped (str.strip()), whitespace-only
 * tokens are dropped.  counts_out[n_str] = tokens per string; spans_out[2*k], spans_out[2*k+1] = [start, end) of token
 * k relative to its string start (tokens of string 0 first).  spans_cap = capacity in tokens; *n_tokens_out = total
 * (host pointer).  LATOK_ERR_INVALID when spans_cap is too small (n_tokens_out still holds the needed count).
 * Synchronous in both pointer modes. */
int latok_token_spans_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                            int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                            int flags, void* stream);

/* ---- UTF-8 ingest (one step before the path: the reference reads CPython's PEP-393 buffer, latok.c:53-55,79) ---------
 * A batch can also be handed over as UTF-8: `utf8` = packed bytes of all strings, `byte_off[n_str + 1]` = byte offset
 * of each string (byte_off[0] == 0).  The library decodes on the device (one code point per lead byte; input must be
 * valid UTF-8, "surrogatepass" forms decode as they are, truncated sequences give U+FFFD) and runs the same pipeline.
 * Each string must itself be valid UTF-8: on malformed input a sequence that a string's end cuts is read on into the
 * following string's bytes (the window of a lead byte is taken from the packed stream), never past the end of the batch.
 * All results are in CODE-POINT units, exactly what the reference would report for the decoded str.  With host
 * pointers this moves 1 byte per ASCII char over PCIe instead of 4. */
int latok_utf8_decode_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                            uint32_t* cps_out, int64_t cps_cap, int64_t* cp_row_off_out, int64_t* total_cps_out, int flags,
                            void* stream);
/* boundary bitmask over the DECODED code points (bit i = code point i of the packed batch) + the code-point row offsets */
int latok_split_mask_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                uint64_t* mask_bits_out, int64_t mask_cap_words, int64_t* cp_row_off_out,
                                int64_t* total_cps_out, int flags, void* stream);
int latok_split_offsets_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                   int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap,
                                   int64_t* n_offsets_out, int flags, void* stream);
int latok_token_spans_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                 int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                 int flags, void* stream);
/* featurize of the decoded text: latok_token_features_batch (below) on what latok_utf8_decode_batch would give -- spans4 in
 * code points relative to each string, the 25 feature sums per token -- with the same flags (LATOK_OUT_INT32, LATOK_DEVICE_PTRS),
 * total_bytes = -1 and capacity protocol; features_out NULL with cap > 0 is refused.  Large well-formed batches make no UTF-32
 * copy: the byte-space pipeline gives the code-point masks and one kernel stores the rule code of every char at its code-point
 * index (1 B/char) for the feature sums.  Malformed input gives what the staged decoder gives. */
int latok_token_features_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                    int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                    int64_t* n_tokens_out, int flags, void* stream);

/* ---- UTF-8 in BYTE space (fused ingest) -----------------------------------------------------------------------------
 * Same tokenization, but nothing is decoded to UTF-32: the tile kernel reads the UTF-8 bytes themselves (1 byte per
 * ASCII char from HBM instead of 4) and every position it reports is a BYTE position in the caller's buffer:
 *   mask     bit i = byte i of the packed buffer; set at the LEAD byte of every char the reference marks as a boundary
 *            (np.nonzero(gen_split_mask(...)), default_tokenizer.py:148), mapped from code-point to byte positions
 *   offsets  byte offsets relative to the start of each string
 *   spans    [start, end) byte ranges of the stripped, non-empty tokens: utf8[byte_off[s] + start : byte_off[s] + end]
 *            is the UTF-8 encoding of the token the reference yields
 *   featurize  the four positions of a token's span record as byte positions, the 25 feature sums per char
 * Input must be valid UTF-8 ("surrogatepass" forms are accepted as they decode); a truncated sequence counts as
 * U+FFFD, stray continuation bytes belong to no char.  With LATOK_DEVICE_PTRS the byte buffer must be 16-byte aligned.
 * Run-time rule tables (latok_set_rules) apply in byte space too (evaluated by the byte-space tile kernel itself). */
int latok_split_mask_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                      uint64_t* mask_bits_out, int flags, void* stream);
int latok_split_offsets_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                         int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap,
                                         int64_t* n_offsets_out, int flags, void* stream);
int latok_token_spans_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                       int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                       int flags, void* stream);

/* featurize in byte space: latok_token_features_batch (below) for a caller who holds bytes and slices bytes.  Token for token
 * (same tokens, same order, same counts) what the two calls above and latok_token_features_utf8_batch report:
 *   spans4_out[4k + 2], [4k + 3]   the stripped BYTE range = the record of latok_token_spans_utf8_bytes_batch (LaToken.text =
 *                                  utf8[byte_off[s] + strip_start : byte_off[s] + strip_end])
 *   spans4_out[4k], [4k + 1]       the raw BYTE range = the two consecutive offsets of latok_split_offsets_utf8_bytes_batch (the
 *                                  string's byte length closing the last one) that enclose it
 *   features_out[25k .. 25k + 24]  the sums latok_token_features_utf8_batch gives for the token: one count per CHAR, not per byte
 * i.e. the reference's featurize of the decoded string with every position mapped from a char to the first byte of that char
 * (end positions: the byte behind the char's last byte).  Flags, total_bytes = -1, the capacity protocol (cap in tokens; too
 * small: nothing written to records or sums, counts valid, needed count in *n_tokens_out; cap = 0 with NULL buffers = size query;
 * features_out NULL with cap > 0 is refused) and run-time rule tables as in latok_token_features_utf8_batch; under LATOK_OUT_INT32
 * a string of 2^31 BYTES or more fails.  Truncated sequences and lone lead bytes count as one char each, as everywhere in byte
 * space.  A batch with a STRAY continuation byte (none of the 3 bytes before it is a lead byte, or it opens a string) has no
 * defined feature sums here -- byte space assigns the byte to no char, the decoder makes it U+FFFD -- and is REFUSED:
 * LATOK_ERR_INVALID ("malformed UTF-8"), no record and no sum written, *n_tokens_out = 0.  Such input can go to
 * latok_token_features_utf8_batch (code-point results through the staged decoder) or to latok_token_spans_utf8_bytes_batch
 * (byte ranges without sums). */
int latok_token_features_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                          int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                          int64_t* n_tokens_out, int flags, void* stream);

/* Joined token text in byte space: the tokens themselves, not positions -- what the reference's tokenize() yields
 * (default_tokenizer.py:149-160), one line per string.  Input as latok_token_spans_utf8_bytes_batch takes it; sep is one byte,
 * any value 0..255 (another value is refused before any device work).  For string s let (a_k, e_k), k = 0 .. c_s - 1, be the
 * records latok_token_spans_utf8_bytes_batch reports for it (stripped, non-empty tokens as byte ranges relative to byte_off[s]):
 *   row(s)       = sep.join(utf8[byte_off[s] + a_k : byte_off[s] + e_k] for k in 0 .. c_s - 1)
 *   out_off[0]   = 0
 *   out_off[s+1] = out_off[s] + len(row(s)) = out_off[s] + sum(e_k - a_k) + max(c_s - 1, 0)
 *   out_bytes[out_off[s] : out_off[s+1]] = row(s)
 *   counts_out[s] = c_s                            (counts_out may be NULL; LATOK_OUT_INT32 applies to it alone, out_off is int64)
 * Under the built-in tables, for a non-empty well-formed string, row(s) = sep.join(tokenize(text)).encode("utf-8") of the
 * reference.  An empty and a whitespace-only string give an empty row (the reference raises on ''; batch mode, see above).  The
 * bytes of a span are copied verbatim and the spans call defines the spans: run-time rule tables, truncated sequences, lone lead
 * bytes and stray continuation bytes need no rule of their own, nothing is refused as malformed.  Every kept token has at least
 * one byte and brings at most one separator, so out_off[n_str] <= 2 * total_bytes ("a,b" -> "a , b"): size buffers by it.
 * Capacity protocol, in BYTES: out_cap too small -> nothing is written to out_bytes, out_off and counts stay valid, the needed
 * size is in *n_out_bytes and the call returns LATOK_ERR_INVALID; out_cap = 0 with out_bytes = NULL is a size query; out_bytes =
 * NULL with out_cap > 0 is refused.  Host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned), total_bytes = -1
 * as in the sibling calls; a flag bit other than these two is refused.  With device pointers the call synchronises once; with
 * host pointers a second time behind the copy of the bytes (their number is known only after the first).  Every batch size takes the
 * same kernels and gives the same bytes. */
int latok_join_tokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                       int sep, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off /* int64[n_str+1] */,
                                       void* counts_out /* may be NULL */, int64_t* n_out_bytes, int flags, void* stream);

/* Token hashes in byte space: one 32-bit id per token instead of positions or text -- what a hashing vectorizer, feature hashing
 * or a hashed embedding table consume.  A token is what the reference's tokenize() yields (default_tokenizer.py:149-160): for
 * string s let (a_k, e_k), k = 0 .. c_s - 1, be the records latok_token_spans_utf8_bytes_batch reports for it (stripped,
 * non-empty tokens as byte ranges relative to byte_off[s]), and rank(s, k) = c_0 + .. + c_(s-1) + k.  Then
 *   hashes_out[rank(s, k)] = MurmurHash3 x86_32 (murmur3_x86_32) of utf8[byte_off[s] + a_k : byte_off[s] + e_k] with `seed`
 *   counts_out[s]          = c_s                        (may be NULL)
 *   spans_out[2 rank(s, k)], [2 rank(s, k) + 1] = a_k, e_k   (may be NULL; the records of the spans call, byte for byte)
 * LATOK_OUT_INT32 applies to counts and spans; a hash is always one uint32.  MurmurHash3 x86_32 is the function of scikit-learn's
 * HashingVectorizer / FeatureHasher, Spark's HashingTF and Vowpal Wabbit: sklearn.utils.murmurhash3_32(token_bytes, seed) is this
 * uint32 read as int32 (the same word with positive=True); bucket reduction (% n, sign) is the consumer's.  The bytes of a span are
 * hashed verbatim and the spans call defines the spans: run-time rule tables, truncated sequences, lone lead bytes and stray
 * continuation bytes need no rule of their own, nothing is refused as malformed.  Empty and whitespace-only strings contribute no
 * token; n_str = 0 or total_bytes = 0 gives zero tokens with counts cleared.
 * Capacity protocol, in TOKENS, as in the spans call: cap too small -> nothing is written to hashes or records, counts stay valid,
 * the needed count is in *n_tokens_out and the call returns LATOK_ERR_INVALID; cap = 0 with hashes_out = NULL is a size query;
 * hashes_out = NULL with cap > 0 is refused.  Host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned; the kernel
 * reads the text as aligned 4-byte words, up to the word that holds the last byte), total_bytes = -1 as in the sibling calls; a
 * flag bit other than these two is refused before any device work.  Every batch size takes the same kernels and gives the same
 * words; the call waits for its kernels once. */
int latok_token_hashes_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                        uint32_t seed, int64_t* counts_out /* may be NULL */, int64_t* spans_out /* may be NULL */,
                                        uint32_t* hashes_out, int64_t cap, int64_t* n_tokens_out, int flags, void* stream);

/* Token ids in byte space: every token's id in a vocabulary -- an index into an embedding table, a count vector or a label space.
 * A VOCABULARY is an ordered list of byte strings w_0 .. w_(V-1).  It may carry ids id_0 .. id_(V-1) (int32; word_ids = NULL means
 * id_i = i) and it carries a 32-bit seed (of the MurmurHash3 x86_32 that places a word in the table; it does not change any id).
 * A token is what the reference's tokenize() yields (default_tokenizer.py:149-160): for string s let (a_k, e_k), k = 0 .. c_s - 1, be
 * the records latok_token_spans_utf8_bytes_batch reports for it, rank(s, k) = c_0 + .. + c_(s-1) + k as for the hashes call, and i
 * the LOWEST index whose word equals the token's bytes utf8[byte_off[s] + a_k : byte_off[s] + e_k], byte for byte and of the same
 * length.  Then
 *   ids_out[rank(s, k)] = id_i      if such an i exists
 *                         unk_id    otherwise (any int32, per call)
 *   counts_out[s]       = c_s                        (may be NULL)
 *   spans_out[2 rank(s, k)], [2 rank(s, k) + 1] = a_k, e_k   (may be NULL; the records of the spans call, byte for byte)
 * Exact: the hash only finds the slot, equality is decided by comparing the bytes, so two different byte strings never share an id
 * because their hashes agree.  Of a duplicate word the first occurrence wins.  The empty word is accepted and never matches (no
 * token is empty).  V = 0 is accepted: every token gets unk_id.  Token bytes are compared verbatim and the spans call defines the
 * spans: run-time rule tables, truncated sequences, lone lead bytes and stray continuation bytes need no rule of their own, nothing
 * is refused as malformed.
 * latok_vocab_create takes HOST pointers (words: the words back to back; word_off[n_words + 1]: their offsets, non-decreasing from
 * 0), builds the table on the host and uploads it to the device of the current context.  Refused before any device work: a
 * word_off that is not non-decreasing from 0, n_words >= 2^31, words that take 2^32 bytes or more once each is padded to 4, NULL
 * outputs.  The object is immutable afterwards: any context of the same device may use it, concurrently; a call whose current
 * context sits on another device returns LATOK_ERR_INVALID.  latok_vocab_destroy drains the current context (its stream and its
 * flow) before it frees -- whatever they report, the object is freed --; as with latok_ctx_destroy, every OTHER context must be done with the object.  latok_vocab_info reports
 * the word count as given, the slot count of the table (a power of two, >= 2 V and >= 64), the seed and the device; any output
 * pointer may be NULL. */
typedef struct latok_vocab latok_vocab;
int latok_vocab_create(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                       const int32_t* word_ids /* may be NULL */, uint32_t seed, latok_vocab** vocab_out);
int latok_vocab_destroy(latok_vocab* vocab);
int latok_vocab_info(const latok_vocab* vocab, int64_t* n_words, int64_t* n_slots, uint32_t* seed, int* device);
/* The ids call follows latok_token_hashes_utf8_bytes_batch in everything that is not the lookup.  LATOK_OUT_INT32 applies to
 * counts and spans; an id is always one int32.  Empty and whitespace-only strings contribute no token; n_str = 0 or total_bytes =
 * 0 gives zero tokens with counts cleared.  Capacity protocol, in TOKENS: cap too small -> nothing is written to ids or records,
 * counts stay valid, the needed count is in *n_tokens_out and the call returns LATOK_ERR_INVALID; cap = 0 with ids_out = NULL is a
 * size query; ids_out = NULL with cap > 0 is refused.  Host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned;
 * the kernel reads the text as aligned 4-byte words, up to the word that holds the last byte), total_bytes = -1 as in the sibling
 * calls; a flag bit other than these two is refused before any device work.  Every batch size takes the same kernels and gives the
 * same ids; the call waits for its kernels once. */
int latok_token_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                     const latok_vocab* vocab, int32_t unk_id, int64_t* counts_out /* may be NULL */,
                                     int64_t* spans_out /* may be NULL */, int32_t* ids_out, int64_t cap, int64_t* n_tokens_out,
                                     int flags, void* stream);

/* Per-string term counts in byte space: the rows of a document-term matrix, as the three arrays of a canonical CSR matrix --
 * what CountVectorizer(vocabulary=...).transform and HashingVectorizer(norm=None).transform return.  A token is what the spans call
 * yields: for string s, t_0 .. t_(c_s-1) are the byte slices latok_token_spans_utf8_bytes_batch reports; run-time rule tables and
 * malformed bytes are taken as that call takes them.  Every token gets a key and a value:
 *   vocabulary form   key = id_i of the lowest-indexed word equal to the token, byte for byte -- exactly the id
 *                     latok_token_ids_utf8_bytes_batch would store --, value = 1.  A token with no such word is OUT OF VOCABULARY:
 *                     it contributes no entry and adds 1 to oov[s].  "Not found" is kept apart from every legal id (a vocabulary
 *                     may carry any int32 as an id: there is no unk sentinel).  Two words that carry the same id count into the
 *                     same entry.  V = 0 is accepted: every token is out of vocabulary.
 *   hashed form       h = MurmurHash3 x86_32 of the token's bytes with `seed`, read as int32; key = |h| mod n_features, computed in
 *                     64 bits (h = -2^31 gives 2^31 mod n_features: scikit-learn's rule in _hashing_fast.pyx); value = (h >= 0 ? +1
 *                     : -1) if alternate_sign, else +1.  n_features must be in 1 .. 2^31 - 1; anything else is refused before
 *                     any device work.
 * Row s is the set of distinct keys of its tokens, ascending as signed int32, each with the sum of its values:
 *   indptr[0] = 0, indptr[s+1] = indptr[s] + (number of distinct keys of string s)
 *   indices[indptr[s] + j] = j-th smallest key of string s
 *   data   [indptr[s] + j] = sum of the values of the tokens of s with that key   (int32)
 *   oov[s]                 = number of out-of-vocabulary tokens of s             (vocabulary form; may be NULL)
 * In the hashed form a sum may be 0: the entry is kept, as scikit-learn keeps it after sum_duplicates.  The output is fully
 * deterministic (unlike the order of latok_counter_read).  Empty strings, whitespace-only strings and all-OOV strings give empty
 * rows; n_str = 0 or total_bytes = 0 gives nnz = 0 with indptr cleared.
 * Everything else follows the ids call: host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned), total_bytes =
 * -1, check of the vocabulary's device; LATOK_OUT_INT32 applies to indptr and oov (an index and a count are always one int32); any
 * other flag bit is refused before any device work.  Capacity protocol, in ENTRIES (nnz): cap too small -> nothing is written to
 * indices or data, indptr and oov stay valid, the need is in *nnz_out and the call returns LATOK_ERR_INVALID; cap = 0 with both
 * buffers NULL is a size query; exactly one of the two NULL, or both NULL with cap > 0, is refused.  A batch whose token total is
 * 2^31 or more is refused with nothing written (data is int32).  *n_tokens_out (may be NULL) = the token total.  Every batch size
 * takes the same kernels.  The calls are blocking and wait for their kernels TWICE -- once for the token total, which sizes the key
 * buffers, once for nnz --, and a third time for the copy of the entries when the outputs are host pointers.  There is no flow
 * form. */
int latok_term_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                       const latok_vocab* vocab, int64_t* indptr_out /* [n_str+1] */,
                                       int64_t* oov_out /* [n_str], may be NULL */, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                       int64_t* nnz_out, int64_t* n_tokens_out /* may be NULL */, int flags, void* stream);
int latok_hashed_term_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                              uint32_t seed, int64_t n_features, int alternate_sign, int64_t* indptr_out /* [n_str+1] */,
                                              int32_t* indices_out, int32_t* data_out, int64_t cap, int64_t* nnz_out,
                                              int64_t* n_tokens_out /* may be NULL */, int flags, void* stream);

/* Word n-grams in the term counts: the same CSR rows with one term per GRAM -- what CountVectorizer(vocabulary=...,
 * ngram_range=(min_n, max_n)) and HashingVectorizer(norm=None, ngram_range=(min_n, max_n)) return; scikit-learn's _word_ngrams
 * feeds exactly these strings to its vocabulary or hasher.  For string s the tokens t_0 .. t_(c-1) are the byte slices
 * latok_token_spans_utf8_bytes_batch reports; run-time rule tables and malformed bytes are taken as that call takes them.  The GRAMS
 * of s, for 1 <= min_n <= max_n <= 8 and a one-byte separator sep (0 .. 255; scikit-learn joins with 0x20), are
 *   g(n, i) = t_i + sep + t_(i+1) + sep + ... + t_(i+n-1)     for every n in [min_n, max_n] and every i in 0 .. c - n
 * -- a string with fewer than n tokens has no gram of order n; a string of c tokens has sum over n of max(0, c - n + 1) grams.
 * Every gram gets a key and a value by exactly the rules of the term-counts comment above, applied to the BYTES OF THE GRAM:
 *   vocabulary form   the gram is looked up byte for byte in the latok_vocab; a vocabulary word may contain the separator
 *                     ("new york").  A found gram contributes its id with value 1; a gram that is not found adds 1 to oov[s].
 *   hashed form       h = MurmurHash3 x86_32 of the gram's bytes with `seed`; column = |h| mod n_features in 64 bits; the sign follows
 *                     alternate_sign; the gram's byte length enters the hash as 32 bits.
 * Row s is the set of distinct keys ascending as signed int32, each with the sum of its values, in the CSR layout above.  With min_n
 * = max_n = 1 the result equals latok_term_counts_utf8_bytes_batch / latok_hashed_term_counts_utf8_bytes_batch entry for entry.
 * Everything else carries over from those calls unchanged: flags, host pointers or LATOK_DEVICE_PTRS, total_bytes = -1, the check
 * of the vocabulary's device, the capacity protocol in ENTRIES, the size query, the empty batch.  min_n < 1, max_n < min_n, max_n >
 * 8 and sep outside 0 .. 255 are refused with LATOK_ERR_INVALID before any device work, with nothing written.  A batch whose token
 * total, or whose gram total K, is 2^31 or more is refused with nothing written to indices or data.  *n_grams_out (may be NULL) = K.
 * The calls are blocking and wait for their kernels THREE times -- for the token total, which sizes the token records; for K,
 * which sizes the key buffers; for nnz -- and a fourth time for the copy of the entries when the outputs are host pointers.  A
 * gram is hashed by one lane: a batch of very long tokens runs at the speed of its longest.  There is no flow form. */
int latok_ngram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                        const latok_vocab* vocab, int min_n, int max_n, int sep, int64_t* indptr_out /* [n_str+1] */,
                                        int64_t* oov_out /* [n_str], may be NULL */, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                        int64_t* nnz_out, int64_t* n_grams_out /* may be NULL */, int flags, void* stream);
int latok_hashed_ngram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                               uint32_t seed, int64_t n_features, int alternate_sign, int min_n, int max_n, int sep,
                                               int64_t* indptr_out /* [n_str+1] */, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                               int64_t* nnz_out, int64_t* n_grams_out /* may be NULL */, int flags, void* stream);

/* Character n-grams inside tokens in the term counts: the same CSR rows with one term per CHARACTER GRAM of every token -- what
 * CountVectorizer(analyzer="char_wb", vocabulary=..., ngram_range=(min_n, max_n)) and HashingVectorizer(analyzer="char_wb", norm=None,
 * ngram_range=(min_n, max_n)) return for " ".join(tokens); scikit-learn's _char_wb_ngrams feeds exactly these strings to its
 * vocabulary or hasher.  The tokens are what latok_token_spans_utf8_bytes_batch reports for string s; run-time rule tables and
 * malformed bytes are taken as that call takes them.
 *   character     a character of a token starts at the token's first byte and at every later byte b with (b & 0xC0) != 0x80.  For
 *                 valid UTF-8 these are the code points; for malformed bytes the rule is still total.  A character's bytes run to the
 *                 next start or to the token's end.
 *   padded word   for a token of L >= 1 characters: pad, c_0 .. c_(L-1), pad -- W = L + 2 characters; pad is one byte, 0 .. 255
 *                 (scikit-learn uses 0x20).
 *   grams         for n from min_n up to max_n, in this order, 1 <= min_n <= max_n <= 8: if n < W, the W - n + 1 runs of n
 *                 neighbouring characters of the padded word; if n >= W, the only gram is the whole padded word, once, and NO HIGHER
 *                 ORDER CONTRIBUTES (scikit-learn: "count a short word only once").
 *   gram count    G(W) = sum over n in [min_n, min(max_n, W - 1)] of (W - n + 1), plus 1 if max_n >= W.  A token whose record is empty
 *                 or does not lie in the text has no gram.  A string's grams are those of its tokens; K is the batch's gram total.
 * Every gram gets a key and a value by exactly the rules of the term-counts comment above, applied to the BYTES OF THE GRAM:
 *   vocabulary form   byte-for-byte lookup in the latok_vocab; a vocabulary word may hold the pad (" th").  A found gram contributes
 *                     its id with value 1; a gram that is not found adds 1 to oov[s].
 *   hashed form       h = MurmurHash3 x86_32 of the gram's bytes with `seed`; column = |h| mod n_features in 64 bits; the sign follows
 *                     alternate_sign.
 * Rows, CSR layout and determinism carry over unchanged, and so do flags, host pointers or LATOK_DEVICE_PTRS, total_bytes = -1, the
 * check of the vocabulary's device, the capacity protocol in ENTRIES with its size query, LATOK_OUT_INT32 and the empty batch.
 * *n_grams_out (may be NULL) = K.  A batch whose token total, or whose K, is 2^31 or more is refused with nothing written to indices or
 * data.  min_n < 1, max_n < min_n, max_n > 8 and pad outside 0 .. 255 are refused with LATOK_ERR_INVALID before any device work, with
 * nothing written.  The calls are blocking and wait for their kernels THREE times, as the word n-gram calls do, and a fourth time for
 * the copy of the entries when the outputs are host pointers.  Every batch size takes the same kernels.  One lane walks a token alone:
 * a batch with very long tokens runs at the speed of its longest; there is no whole-wave form for long tokens.
 * Not built: the plain analyzer="char" (over the whole string, with scikit-learn's whitespace collapsing: it needs no tokenizer);
 * one-call TF-IDF and idf-update forms (the composition of these counts with latok_idf_update_csr and latok_tfidf_csr works with
 * device pointers and no host visit); fitting a gram vocabulary; a flow form. */
int latok_chargram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                           const latok_vocab* vocab, int min_n, int max_n, int pad, int64_t* indptr_out /* [n_str+1] */,
                                           int64_t* oov_out /* [n_str], may be NULL */, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                           int64_t* nnz_out, int64_t* n_grams_out /* may be NULL */, int flags, void* stream);
int latok_hashed_chargram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                                  uint32_t seed, int64_t n_features, int alternate_sign, int min_n, int max_n, int pad,
                                                  int64_t* indptr_out /* [n_str+1] */, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                                  int64_t* nnz_out, int64_t* n_grams_out /* may be NULL */, int flags, void* stream);

/* TF-IDF on the device: document frequencies over many batches, and the float32 weighting of CSR rows -- what TfidfTransformer /
 * TfidfVectorizer add to the term counts above, and the norm="l2" / "l1" of HashingVectorizer.
 * A latok_idf is a mutable device object like latok_counter: int32 df[n_cols] (in how many rows a column was stored) and int64 n_docs
 * (rows seen), on the device of the context that created it; every call checks that device against the current context's.  Calls on
 * one object are serialised by a lock inside it.  latok_idf_create: n_cols in 1 .. 2^28, anything else is refused before any device
 * work; df and n_docs start at zero.  latok_idf_info needs no device call; any output pointer may be NULL.  latok_idf_clear zeroes
 * df and n_docs.  latok_idf_destroy drains the current context (its stream and its flow) first, like latok_vocab_destroy.
 *   latok_idf_update_csr   df[c] += 1 for every STORED entry with column c, n_docs += n_rows: np.bincount(X.indices, minlength=n_cols)
 *                          of a CSR matrix, scikit-learn's _document_frequency.  Explicit zeros count (the hashed rows keep them, as
 *                          scikit-learn does).  A row's columns are taken as distinct, as every CSR of this library has them; the call
 *                          does not check that.  Host pointers or LATOK_DEVICE_PTRS; LATOK_OUT_INT32: indptr is int32, else int64; any
 *                          other flag bit is refused.  The CSR is validated on the device before df is touched: indptr[0] = 0,
 *                          non-decreasing, indptr[n_rows] = nnz, every index in [0, n_cols) -- a vocabulary may carry any int32 as an
 *                          id, so an out-of-range column is a real case.  A refused call leaves df and n_docs exactly as they were.
 *                          The call is refused when n_docs + n_rows would reach 2^31 (df is int32).  Blocking.
 *   latok_idf_update_utf8_bytes_batch
 *                          the same update straight from text: the term-count pipeline of the calls above (vocab, or vocab = NULL:
 *                          the hashed form with seed and n_features; min_n = max_n = 1: the plain term counts, else word n-grams
 *                          joined by sep) runs into the context's own buffers and its indptr / indices feed the update; no entry
 *                          visits the host.  Hashed form: n_features must equal n_cols, else the call is refused before any device work
 *                          (alternate_sign has no bearing on which entries exist and is not an argument).  Vocabulary form: an id
 *                          outside [0, n_cols) refuses the call with df and n_docs unchanged.  n_docs += n_str, empty strings
 *                          included.  Flags: LATOK_DEVICE_PTRS only.  *nnz_out, *n_tokens_out (may be NULL) as in the count calls.
 *   latok_idf_read         df to HOST pointers with the size-query protocol of latok_counter_read: *n_docs_out (may be NULL) is always
 *                          set; cap = 0 with df_out NULL is a size query that returns LATOK_OK; 0 < cap < n_cols writes nothing and
 *                          returns LATOK_ERR_INVALID (the need is n_cols: latok_idf_info).
 *   latok_idf_load         sets df[n_cols] and n_docs from HOST pointers, for an idf that was fitted elsewhere; refused with nothing
 *                          changed if n_docs is negative or 2^31 or more, or any df[c] lies outside [0, n_docs].
 *   latok_idf_weights      the idf vector to HOST pointers (cap >= n_cols floats):
 *                            idf[c] = ln((n_docs + s) / (df[c] + s)) + 1,  s = 1 if smooth else 0
 *                          evaluated in double on the device and rounded once to float32.  WITHOUT smoothing a column with df[c] = 0
 *                          gets idf[c] = 0, where scikit-learn divides by zero.  The vector is computed once per smoothing mode and
 *                          kept until the next update, load or clear.
 * Multi-device: there is no merge call; latok_idf_read on every device, a sum on the host and latok_idf_load is the route.
 *
 * latok_tfidf_csr is TfidfTransformer.transform on a CSR in host or device memory (flags as latok_idf_update_csr): int32 counts in,
 * float32 weights out; data_out may be `data` itself.  idf = NULL: no idf.  opts is an OR of LATOK_TFIDF_*; both norm bits together,
 * or an unknown bit, are refused before any device work.  For entry j of row r with count t and column c:
 *   tf  = t; with LATOK_TFIDF_SUBLINEAR_TF: sign(t) * (1 + ln|t|) for t != 0, and 0 for t = 0.  (scikit-learn takes ln of the stored
 *         value and gives NaN for the negative and zero sums of alternate_sign; this definition agrees with it wherever it is defined.)
 *   w   = tf * idf[c] (LATOK_TFIDF_SMOOTH_IDF picks the smoothing mode), or tf without an idf
 *   out = w / N_r,  N_r = sqrt(sum of w^2) with LATOK_TFIDF_NORM_L2, sum of |w| with LATOK_TFIDF_NORM_L1, 1 with neither
 * A row whose norm is 0 keeps its zeros; an entry with t = 0 is exactly 0.0f; no NaN or infinity comes from finite input.  A row's
 * output bits depend on that row alone -- its (indices, data) in order, the idf of its columns, opts -- not on its place in the
 * batch, its neighbours, the batch size or host versus device pointers: a fixed group of lanes chosen by the row's length sums in a
 * fixed order, and there is no floating-point atomic.  Every output lies within (k + 16) * 2^-23 relative of the exact value for a
 * normalised row of k stored entries and within 8 * 2^-23 without a norm; a single-entry row under L2 with a nonzero weight is exactly
 * +-1.0f.  The CSR is validated as in latok_idf_update_csr, the columns only when idf is given; a refused call writes nothing to
 * data_out.  Blocking.
 *
 * latok_tfidf_utf8_bytes_batch / latok_hashed_tfidf_utf8_bytes_batch: text to TF-IDF rows in one call.  indptr, indices and oov are
 * entry for entry those of latok_ngram_counts_utf8_bytes_batch / latok_hashed_ngram_counts_utf8_bytes_batch with the same arguments
 * (min_n = max_n = 1 takes the plain term counts' kernels); data_out is the weighting of their data, bit for bit what
 * latok_tfidf_csr gives on that CSR.  The weighting runs on the device behind the counts, in place, and adds no wait to theirs.
 * Everything else carries over: the capacity protocol in ENTRIES with its size query, LATOK_OUT_INT32, LATOK_DEVICE_PTRS,
 * total_bytes = -1, the empty batch, the refusal of 2^31 tokens or grams, the n-gram argument checks.  idf may be NULL.  Hashed form
 * with an idf: n_features != n_cols is refused before any device work.  Vocabulary form with an idf: an id outside [0, n_cols)
 * refuses the call behind its kernels; host output buffers are then untouched, device output buffers hold the unweighted counts. */
#define LATOK_TFIDF_SMOOTH_IDF 1
#define LATOK_TFIDF_SUBLINEAR_TF 2
#define LATOK_TFIDF_NORM_L1 4
#define LATOK_TFIDF_NORM_L2 8
typedef struct latok_idf latok_idf;
int latok_idf_create(int64_t n_cols, latok_idf** out);
int latok_idf_destroy(latok_idf* idf);
int latok_idf_clear(latok_idf* idf);
int latok_idf_info(const latok_idf* idf, int64_t* n_cols, int64_t* n_docs, int* device);
int latok_idf_update_csr(latok_idf* idf, const void* indptr /* [n_rows+1] */, const int32_t* indices, int64_t n_rows, int64_t nnz,
                         int flags, void* stream);
int latok_idf_update_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                      const latok_vocab* vocab /* NULL: hashed */, uint32_t seed, int64_t n_features, int min_n, int max_n,
                                      int sep, latok_idf* idf, int64_t* nnz_out /* may be NULL */, int64_t* n_tokens_out /* may be NULL */,
                                      int flags, void* stream);
int latok_idf_read(const latok_idf* idf, int32_t* df_out, int64_t cap, int64_t* n_docs_out);
int latok_idf_load(latok_idf* idf, const int32_t* df /* [n_cols] */, int64_t n_docs);
int latok_idf_weights(const latok_idf* idf, int smooth, float* out, int64_t cap);
int latok_tfidf_csr(const void* indptr /* [n_rows+1] */, const int32_t* indices, const int32_t* data, int64_t n_rows, int64_t nnz,
                    const latok_idf* idf /* NULL: no idf */, int opts, float* data_out, int flags, void* stream);
int latok_tfidf_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                 const latok_vocab* vocab, int min_n, int max_n, int sep, const latok_idf* idf /* may be NULL */, int opts,
                                 int64_t* indptr_out /* [n_str+1] */, int64_t* oov_out /* [n_str], may be NULL */, int32_t* indices_out,
                                 float* data_out, int64_t cap, int64_t* nnz_out, int flags, void* stream);
int latok_hashed_tfidf_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                        int64_t n_features, int alternate_sign, int min_n, int max_n, int sep,
                                        const latok_idf* idf /* may be NULL */, int opts, int64_t* indptr_out /* [n_str+1] */,
                                        int32_t* indices_out, float* data_out, int64_t cap, int64_t* nnz_out, int flags, void* stream);

/* WordPiece in byte space: the subword ids a BERT-family model takes, for every token of a batch.
 * A WORDPIECE VOCABULARY is an ordered list of byte strings w_0 .. w_(V-1) with optional int32 ids (word_ids = NULL means id_i = i),
 * a continuation prefix P of 0 .. 8 bytes ("##" in BERT's files; an empty P is legal: every word is then also a continuation word),
 * a 32-bit seed (of the MurmurHash3 x86_32 that places a word; it changes no id) and max_chars in 1 .. 1024 (BERT's
 * max_input_chars_per_word).  It is one immutable device object that holds two tables of the kind latok_vocab holds: the INITIAL
 * table holds every word; the CONTINUATION table holds every word that starts with P and is longer than P, stored without P, with
 * the same id.  Of duplicate words the first wins.  These are exactly the lookups of one dictionary that gets `piece` at a token's
 * start and P + piece elsewhere.  Each table records the byte length of its longest word.
 * A token is what the spans call yields: bytes [a, e) of string s from latok_token_spans_utf8_bytes_batch; run-time rule tables and
 * malformed bytes are taken as that call takes them.  A CHAR START is the token's first byte, and any later byte b with
 * (b & 0xC0) != 0x80; chars(token) is the number of char starts.  The cut, per token:
 *   1. chars(token) > max_chars: the token is ONE piece (unk_id, a, e).
 *   2. otherwise start = a; while start < e:
 *        among the ends p in (start, e] where p == e or p is a char start, take the LARGEST p such that bytes[start:p] is a word of
 *        the initial table (if start == a) or of the continuation table (otherwise), compared byte for byte;
 *        no end matches: the WHOLE token is one piece (unk_id, a, e), pieces found so far are discarded;
 *        otherwise emit (id, start, p) and set start = p.
 * Exact as the ids call is: the hash finds the slot, the bytes decide.  V = 0 is accepted: every token is one unk piece.  A token
 * that is itself a word gives one piece with the id latok_token_ids_utf8_bytes_batch would give.
 * With c_s tokens in string s and the pieces of a batch numbered in the order of strings, tokens and pieces:
 *   indptr[0] = 0, indptr[s+1] = indptr[s] + (pieces of the tokens of string s)
 *   ids_out[r]                            = the id of piece r (int32)
 *   spans_out[2 r], spans_out[2 r + 1]    = its byte range, relative to its string's first byte (may be NULL)
 * latok_wordpiece_create takes HOST pointers as latok_vocab_create does and refuses, before any device work, what that call refuses
 * and a prefix_len outside 0 .. 8 or a max_chars outside 1 .. 1024.  The object may be used by any context of its device,
 * concurrently; latok_wordpiece_destroy drains the current context first, like latok_vocab_destroy: whatever its stream and
 * its flow report, the object is freed.  latok_wordpiece_info reports the
 * word count as given, the slots and the longest word of both tables, the prefix (8 bytes are written), max_chars, the seed and the
 * device; any output pointer may be NULL.
 * The calls follow the term-counts call: host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned), total_bytes =
 * -1, check of the vocabulary's device; LATOK_OUT_INT32 applies to indptr and spans (an id is always one int32); any other flag bit
 * is refused before any device work.  Capacity protocol, in PIECES: cap too small -> nothing is written to ids or spans, indptr
 * stays valid, the need is in *n_pieces_out and the call returns LATOK_ERR_INVALID; cap = 0 with ids_out = NULL is a size query;
 * ids_out = NULL with cap > 0 is refused.  A batch with 2^31 pieces or more is refused.  *n_tokens_out (may be NULL) = the token
 * total.  n_str = 0 or total_bytes = 0 gives zero pieces with indptr cleared.  Every batch size takes the same kernels.  The
 * calls are blocking: they wait once for the token total, which sizes the token buffers, once for the piece total, and once more
 * for the copy of the pieces when the outputs are host pointers.
 * The PADDED form writes what a model takes: input_ids_out is an [n_str, max_length] block of int32, row s = cls_id (if
 * add_special), the first max_length - 2 add_special pieces of string s, sep_id (if add_special), then pad_id; lengths_out[s]
 * (int32 in every mode) = the cells of row s in front of the padding.  max_length must be >= 1 + 2 add_special, else the call is
 * refused; *n_pieces_out (may be NULL) = the untruncated piece total.  n_str = 0 writes nothing; total_bytes = 0 gives rows of
 * specials and padding.  It waits for the piece total before it sizes its ids, so it waits three times.
 * Lower-casing, accent stripping, control-character cleaning and CJK spacing (the normalizer of BERT's BasicTokenizer) are a call of
 * their own, latok_fold_utf8_bytes_batch below: its output, left on the device, is this call's input, and an uncased vocabulary is
 * served by folding first.  Out of scope: the punctuation split of BERT's BasicTokenizer -- tokens are latok's --, the final-sigma
 * rule of lower-casing, a flow form, sentence pairs.  Byte-level BPE and Unigram models are calls of their own: latok_bpe_* and
 * latok_unigram_* below. */
typedef struct latok_wordpiece latok_wordpiece;
int latok_wordpiece_create(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                           const int32_t* word_ids /* may be NULL */, const uint8_t* prefix, int prefix_len, int max_chars, uint32_t seed,
                           latok_wordpiece** wp_out);
int latok_wordpiece_destroy(latok_wordpiece* wp);
int latok_wordpiece_info(const latok_wordpiece* wp, int64_t* n_words, int64_t* n_slots_initial, int64_t* n_slots_cont,
                         int64_t* max_len_initial, int64_t* max_len_cont, uint8_t* prefix_out /* [8] */, int* prefix_len, int* max_chars,
                         uint32_t* seed, int* device);
int latok_wordpiece_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                         const latok_wordpiece* wp, int32_t unk_id, int64_t* indptr_out /* [n_str+1] */, int32_t* ids_out,
                                         int64_t* spans_out /* may be NULL */, int64_t cap, int64_t* n_pieces_out,
                                         int64_t* n_tokens_out /* may be NULL */, int flags, void* stream);
int latok_wordpiece_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                            const latok_wordpiece* wp, int32_t unk_id, int64_t max_length, int add_special, int32_t cls_id,
                                            int32_t sep_id, int32_t pad_id, int32_t* input_ids_out /* [n_str*max_length] */,
                                            int32_t* lengths_out /* [n_str] */, int64_t* n_pieces_out /* may be NULL */, int flags,
                                            void* stream);

/* Byte-level BPE in byte space: the merge-rank ids a GPT-family model takes (GPT-2 / RoBERTa, the .tiktoken files of the newer
 * models), for every token of a batch.
 * A BPE VOCABULARY is an ordered list of byte strings w_0 .. w_(V-1), in the words / word_off layout latok_vocab_create takes.  The
 * RANK of a word is its position in the list; of duplicates the first wins, so the lowest rank is kept; the empty word gets no slot.
 * word_ids is an optional int32 array (NULL means id = rank); every int32 is a legal id.  The 32-bit seed places the words in the
 * table and changes no id.  max_bytes is in 1 .. 4096, lead_space is 0 or 1.  This is tiktoken's model: a .tiktoken file is exactly
 * such a list, and GPT-2's vocab.json + merges.txt convert to one.  The object is one immutable table of the kind latok_vocab holds
 * (the slot holds the rank), an int32 array rank -> id and the byte length of the longest word.
 * A token is what latok_token_spans_utf8_bytes_batch yields: bytes [a, e) of string s.  With lead_space = 1 a token with a > 0
 * (string-relative) whose byte a - 1 is 0x20 is taken as [a - 1, e): the " word" convention of GPT-style vocabularies.  Any other
 * whitespace is dropped, as everywhere else in the library.  The cut, per token T = bytes[a:e], L = e - a:
 *   1. L > max_bytes: ONE piece (unk_id, a, e).
 *   2. T is a word: ONE piece (id(T), a, e) -- tiktoken's shortcut; step 3 does not imply it (a word need not be reachable by merges).
 *   3. otherwise the parts are the L single bytes.  Repeat: among all ADJACENT parts (p_i, p_(i+1)) whose concatenation is a word,
 *      take the pair whose concatenation has the LOWEST rank; of equal ranks (the same bytes at several places) the LEFTMOST;
 *      replace the two parts by their concatenation.  Stop when no adjacent pair concatenates to a word.
 *   4. emit every remaining part in order as (id, start, end).  A part that is not a word emits unk_id: this can only be a single
 *      byte, since every merged part is a word by construction.  The other parts keep their ids: a token is NOT withdrawn as a whole,
 *      unlike WordPiece.
 * Bytes are bytes: nothing looks at UTF-8 structure, and a character may be split across pieces.  V = 0 is accepted: every token
 * becomes L unk pieces, or one when L > max_bytes.  Exact as the ids call is: the hash finds the slot, the bytes decide.
 * latok_bpe_create takes HOST pointers and refuses, before any device work, what latok_vocab_create refuses and a max_bytes outside
 * 1 .. 4096 or a lead_space other than 0 / 1.  The object may be used by any context of its device, concurrently;
 * latok_bpe_destroy drains the current context first, like latok_vocab_destroy.  latok_bpe_info reports the word count as given, the
 * slots, the longest word, max_bytes, lead_space, the seed and the device; any output pointer may be NULL.
 * The two calls have the contract of the WordPiece calls above, word for word: indptr / ids / spans as there, host pointers or
 * LATOK_DEVICE_PTRS, total_bytes = -1, the check of the object's device, LATOK_OUT_INT32 for indptr and spans, any other flag bit
 * refused before any device work; the capacity protocol in PIECES (cap too small: nothing is written to ids or spans, indptr stays
 * valid, the need is in *n_pieces_out, LATOK_ERR_INVALID; cap = 0 with ids_out = NULL is a size query; ids_out = NULL with cap > 0 is
 * refused); a batch with 2^31 pieces or more is refused; n_str = 0 or total_bytes = 0 as there.  The PADDED form writes the
 * [n_str, max_length] int32 block with bos_id / eos_id where the WordPiece call puts cls_id / sep_id (add_special), and lengths_out.
 * GPT-2's regex pre-tokenizer is a property of the object: latok_bpe_create_pretok with LATOK_PRETOK_GPT2 (below) makes one whose two
 * calls cut the text into GPT-2's pre-tokens instead of latok's tokens -- whitespace runs are encoded, nothing is dropped -- and then
 * merge each as above; an object of latok_bpe_create keeps latok's tokens.  A vocab.json / merges.txt pair converts to the word list
 * on the host (latok_amd.batch.BPE.from_gpt2_files does it).  Out of scope: special-token strings inside the text, folding inside the
 * call, a flow form, decoding ids back to text.  (Decoding is a call family of its own: latok_detok_* below; so are Unigram models:
 * latok_unigram_*.) */
typedef struct latok_bpe latok_bpe;
int latok_bpe_create(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                     const int32_t* word_ids /* may be NULL */, int max_bytes, int lead_space, uint32_t seed, latok_bpe** bpe_out);
int latok_bpe_destroy(latok_bpe* bpe);
int latok_bpe_info(const latok_bpe* bpe, int64_t* n_words, int64_t* n_slots, int64_t* max_len, int* max_bytes, int* lead_space,
                   uint32_t* seed, int* device);
int latok_bpe_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_bpe* bpe,
                                   int32_t unk_id, int64_t* indptr_out /* [n_str+1] */, int32_t* ids_out,
                                   int64_t* spans_out /* may be NULL */, int64_t cap, int64_t* n_pieces_out,
                                   int64_t* n_tokens_out /* may be NULL */, int flags, void* stream);
int latok_bpe_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                      const latok_bpe* bpe, int32_t unk_id, int64_t max_length, int add_special, int32_t bos_id,
                                      int32_t eos_id, int32_t pad_id, int32_t* input_ids_out /* [n_str*max_length] */,
                                      int32_t* lengths_out /* [n_str] */, int64_t* n_pieces_out /* may be NULL */, int flags,
                                      void* stream);

/* GPT-2's pre-tokenizer in byte space: the pre-tokens of GPT-2, RoBERTa, BART and the r50k / p50k encodings, and byte-level BPE behind
 * them -- the ids GPT2TokenizerFast gives.  The pattern is GPT-2's,
 *     's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+
 * applied to each string on its own, leftmost match first, alternatives in order.  Every byte of a string lies in exactly one
 * pre-token; nothing is dropped.  Pre-tokens are byte ranges [a, e) relative to their string.  No regex engine runs: the pattern is
 * restated as a LOCAL rule, which is the definition here (latok_amd/csrc/pretok.h implements it; Unicode 13.0.0):
 * CHARACTERS.  A character starts at a string's first byte and at every later byte b with (b & 0xC0) != 0x80.
 * CLASSES.  Every byte of a character carries that character's class.  If the character's bytes are exactly one well-formed UTF-8
 *   sequence, the class is that of its code point: S = Unicode White_Space (U+0009-000D, 0020, 0085, 00A0, 1680, 2000-200A, 2028,
 *   2029, 202F, 205F, 3000: 25 code points; U+001C-001F are not in it), L = general category L*, N = general category N*, O =
 *   everything else, unassigned code points included.  Any other character is O: a stray continuation byte at a string's start, a
 *   truncated or overlong sequence, a sequence followed by further continuation bytes, a surrogate, a value above U+10FFFF, F5 .. FF.
 * STARTS.  With prev / next the neighbouring characters of the same string, a pre-token starts at character i by these rules:
 *   1. Contractions.  An apostrophe (the one-byte character 0x27) at i is a SCAN START if i is the string's first character, or prev
 *      is L or N, or prev is S and is not the byte 0x20.  A scan-start apostrophe opens a CONTRACTION of k = 2 or 3 bytes if it is
 *      followed by one of s, t, re, ve, m, ll, d -- lower-case ASCII, whole characters (byte i + k, if the string has it, starts a
 *      character), inside the string.  A contraction has no start at its bytes i + 1 .. i + k - 1 and a FORCED start at i + k if
 *      that byte lies inside the string.
 *   2. An S character starts a pre-token if it is the string's first character, or prev is not S, or next exists and is not S (the
 *      last character of a whitespace run in front of text: the lead space of what follows, or a pre-token of its own), or it is forced.
 *   3. A character that is not S and not inside a contraction starts a pre-token if it is the string's first character, or it is
 *      forced, or prev is S and is not the byte 0x20, or prev is not S and its class differs from this character's.  After a 0x20
 *      there is no start: the space is this pre-token's first byte.
 *   4. A string's end ends its last pre-token.  Nothing looks across a string boundary.
 * A start bit depends on the bytes from 7 behind it to 6 ahead of it and on nothing else; latok_set_rules has no influence.
 * latok_pretokens_utf8_bytes_batch has the contract of latok_token_spans_utf8_bytes_batch, word for word (host pointers or
 * LATOK_DEVICE_PTRS with a 16-byte aligned buffer, total_bytes = -1, LATOK_OUT_INT32, the capacity protocol, n_str = 0 and total_bytes
 * = 0), with one argument more: pretok = LATOK_PRETOK_LATOK returns exactly what that call returns, LATOK_PRETOK_GPT2 the pre-tokens
 * above (counts_out[s] = pre-tokens of string s, spans_out = their [a, e) records; every batch size takes the same kernels).  Any
 * other pretok, and any flag bit but those two, is refused before any device work.
 * latok_bpe_create_pretok is latok_bpe_create with the pre-tokenizer as a property of the model, as in a tokenizer.json; it refuses
 * an unknown pretok, and LATOK_PRETOK_GPT2 with lead_space = 1 (the space is already in the pre-token), before any device work.
 * latok_bpe_create means LATOK_PRETOK_LATOK.  latok_bpe_pretokenizer reports it.  The two BPE calls dispatch on the object.
 * Known difference from tiktoken: a pre-token of more than max_bytes (at most 4096) bytes is ONE unk piece, e.g. a run of 5 000
 * spaces, which tiktoken would encode.
 * Out of scope here: the cl100k_base pattern is LATOK_PRETOK_CL100K, defined behind latok_bpe_pretokenizer below (case-insensitive
 * contractions, digits in groups of three, \r\n handling); the o200k_base pattern is not there either.  Also add_prefix_space, special-token
 * strings recognised inside the text, a flow form, folding inside the call, DevicePool forms, this pre-tokenizer on the hash, ids,
 * count, term-count, WordPiece or Unigram calls (the planes make it possible; it is not wired), a Detokenizer loader for GPT-2 files. */
#define LATOK_PRETOK_LATOK 0
#define LATOK_PRETOK_GPT2 1
int latok_pretokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int pretok,
                                     int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out, int flags,
                                     void* stream);
int latok_bpe_create_pretok(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                            const int32_t* word_ids /* may be NULL */, int max_bytes, int lead_space, int pretok, uint32_t seed,
                            latok_bpe** bpe_out);
int latok_bpe_pretokenizer(const latok_bpe* bpe, int* pretok);

/* The cl100k / Llama 3 pre-tokenizer in byte space: the pre-tokens of cl100k_base (GPT-3.5, GPT-4) and of Llama 3, and byte-level BPE
 * behind them.  pretok = LATOK_PRETOK_CL100K (3; the value 2 is reserved and refused) in latok_pretokens_utf8_bytes_batch and
 * latok_bpe_create_pretok, with the contracts stated above; lead_space = 1 is refused as for LATOK_PRETOK_GPT2.  The pattern is
 *     (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
 * applied to each string on its own, leftmost match first, alternatives in order.  No regex engine runs: the rule below is the
 * definition (latok_amd/csrc/pretok.h implements it).  CHARACTERS and CLASSES are those of the GPT-2 rule above (Unicode 13.0.0;
 * malformed characters are O).  NL is the characters CR (0x0D) and LF (0x0A), both S; SP is the byte 0x20; prev / next are the
 * neighbouring characters of the same string; open(i) holds when i is the string's first character or prev is neither O nor SP.
 *   1. Contractions.  An apostrophe (0x27) at i with open(i) opens a contraction if it is followed by one of s t m d re ve ll, the
 *      ASCII letters in either case and any mix, or by U+017F (LATIN SMALL LETTER LONG S, bytes C5 BF: the only other character
 *      that (?i) admits) -- whole characters, inside the string.  The contraction is 2 or 3 bytes; it has no start inside it and a
 *      FORCED start at the byte behind it if the string has one.
 *   2. L at i (not first, not forced, not inside a contraction) starts a pre-token if prev is N, or prev is NL, or prev is O and
 *      open(prev) is false.  After L, after S that is not NL (the pre-token's first character) and after an O with open(prev)
 *      (likewise) there is no start.
 *   3. N at i starts a pre-token if prev is not N or d(i) % 3 == 0, d(i) = the number of N characters (not bytes) that directly
 *      precede i in an unbroken run inside the string.
 *   4. O at i starts a pre-token if open(i).
 *   5. S at i, with absorbed(i) = i is NL and (prev is O or absorbed(prev)), and nl_ahead(i) = i is NL or (next is S and
 *      nl_ahead(next)): no start if absorbed(i); else a start if i is first or prev is not S; else a start if absorbed(prev); else a
 *      start if (prev is NL and not nl_ahead(i)) or (next exists, is not S, and i is not NL).
 *   6. A string's end ends its last pre-token.  Nothing looks across a string boundary: d, absorbed and nl_ahead reset there.
 * E.g. "!\n\n  \n x 1234567  \t!" is cut into "!\n\n", "  \n", " x", " ", "123", "456", "7", "  ", "\t", "!".
 * d, absorbed and nl_ahead reach as far as a run of characters goes (and so does open(prev) across ONE malformed character of any
 * length); everything else depends on at most 8 bytes behind a position and 6 ahead.  The device carries the four across words, tiles
 * and workgroups by composing small records, in two launches and without waiting; latok_set_rules has no influence.
 * The known difference from tiktoken for pre-tokens of more than max_bytes bytes stands (it matters for whitespace runs above 4096
 * bytes).  Out of scope: the o200k_base pattern (letter case structure, \p{M}), special-token strings recognised inside the text,
 * add_prefix_space, a flow form, folding inside the call, DevicePool forms, this pre-tokenizer on the hash, ids, count, term-count,
 * WordPiece or Unigram calls. */
#define LATOK_PRETOK_CL100K 3

/* SentencePiece BPE in byte space: the ids of a SentencePiece model of type BPE (the tokenizer.model of Llama 2, Code Llama, Mistral 7B,
 * Mixtral, TinyLlama, Yi), with byte fallback.  It differs from the byte-level BPE above in four ways: it merges CHARACTERS, not bytes;
 * it has NO whole-token shortcut; every U+0020 becomes the marker U+2581 (bytes E2 96 81), one more marker stands in front of the string,
 * and merges run through runs of markers; a character that no word covers becomes one piece per byte.  The rule below is the definition
 * (latok_amd/csrc/spbpe.h implements it; tests/helpers/spbpe_ref.py restates it).
 *   CHARACTERS  as everywhere: a character starts at a range's first byte and at every later byte b with (b & 0xC0) != 0x80.  The rule
 *               is total on malformed bytes.
 *   SPACE-LIKE  a character whose bytes are exactly 20, or exactly E2 96 81.
 *   SEGMENTS    LATOK_PRETOK_SPM (5; the values 2 and 4 are reserved and refused) in latok_pretokens_utf8_bytes_batch: a segment starts at
 *               a string's first byte, and at every space-like character whose previous character in the same string is not space-like.
 *               Every byte lies in exactly one segment and nothing is dropped; tabs and newlines are ordinary characters.  So a segment is
 *               a (possibly empty) LEAD RUN of space-like characters followed by characters that are not.  A start bit depends on 3 bytes
 *               behind it and 3 ahead: no carry, one launch.  An empty string has no segment.  Route 32.
 *   VIRTUAL TEXT of a segment: one E2 96 81 if the object has add_dummy_prefix and the segment is its string's first; then one E2 96 81
 *               per character of the lead run; then the remaining bytes verbatim.  Its VIRTUAL LENGTH is in bytes.
 *   THE CUT     1. virtual length > max_bytes (1 .. 4096): ONE piece (unk_id, a, e) -- the known difference that the other BPE calls
 *               document.  2. The parts are the CHARACTERS of the virtual text.  There is no whole-segment shortcut: a word that no
 *               sequence of merges reaches is never produced.  3. Repeat: among all adjacent parts whose concatenation is a word, the pair
 *               with the lowest rank (position in the word list), of equal ranks the leftmost, becomes one part; stop when no adjacent pair
 *               is a word.  4. The parts in order: a part that is a word is a piece with its id; a part that is no word is a single
 *               character: with byte_ids one piece per byte b of that character, byte_ids[b]; without byte_ids one unk_id piece, and with
 *               fuse_unk = 1 every maximal run of neighbouring unknown parts of a segment is ONE piece.
 *   SPANS       string-relative bytes.  A virtual character maps to a real range: the dummy marker to the empty range at the segment's
 *               start, the j-th lead marker to the bytes of the j-th lead character (1 or 3), any other character to its own bytes.  A
 *               piece reports from the start of its first character's range to the end of its last character's; every byte piece
 *               reports its character's range; a fused unk the union of its parts' ranges.
 *   PARITY      for well-formed UTF-8 and a model that passes the loader's checks the ids equal SentencePieceProcessor.encode, but for
 *               segments over max_bytes and for distinct words with exactly equal scores (list order here, position in SentencePiece;
 *               trained models have no such ties among merge results).  Malformed input follows the rule above, where SentencePiece
 *               would substitute U+FFFD.
 * Cutting a string into independent segments is exact as long as no word holds E2 96 81 directly behind a character that is not
 * E2 96 81 (true of every model trained with SentencePiece's default split_by_whitespace); latok_bpe_create_spm checks it.
 * latok_bpe_create_spm makes a latok_bpe object of this kind: words / word_off / word_ids as latok_bpe_create takes them (rank = position),
 * byte_ids[256] or NULL (no byte fallback), add_dummy_prefix and fuse_unk 0 or 1.  It refuses, before any device work, what
 * latok_bpe_create refuses, a flag outside 0 / 1 and a word that breaks the condition above (the message names its position).
 * latok_bpe_create_pretok goes on refusing 5: byte merges over these segments mean nothing.  latok_bpe_pretokenizer reports 5 for such
 * an object, latok_bpe_info lead_space = 0; latok_bpe_spm_info reports the three properties and returns LATOK_ERR_INVALID for an object
 * of another kind.  latok_bpe_ids_utf8_bytes_batch and latok_bpe_padded_utf8_bytes_batch dispatch on the object with their contracts
 * unchanged (routes 30 / 31); a batch of this kind has at most 3 * (total_bytes + n_str) pieces.  Objects of latok_bpe_create and
 * latok_bpe_create_pretok take exactly the kernels they took before.
 * Out of scope: NFKC and other normalizers, USER_DEFINED pieces, a decoder mode that turns the marker back into spaces, a BOS-only
 * padded layout, special-token strings inside the text, a flow form, folding inside the call, DevicePool forms. */
#define LATOK_PRETOK_SPM 5
int latok_bpe_create_spm(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                         const int32_t* word_ids /* may be NULL */, const int32_t* byte_ids /* [256], NULL: no byte fallback */,
                         int add_dummy_prefix, int fuse_unk, int max_bytes, uint32_t seed, latok_bpe** bpe_out);
int latok_bpe_spm_info(const latok_bpe* bpe, int* byte_fallback, int* add_dummy_prefix, int* fuse_unk);

/* Unigram in byte space: the Viterbi piece ids of a SentencePiece Unigram language model (T5, mT5, ALBERT, XLNet, XLM-R, mBART,
 * Pegasus), for every token of a batch.
 * THE VOCABULARY.  A Unigram vocabulary is an ordered list of byte strings w_0 .. w_(V-1) in the words / word_off layout of
 * latok_vocab_create.  scores[V] is a float32 array; every score must be finite, else the create call refuses.  word_ids is optional;
 * NULL means id = position.  Of duplicate words the first wins.  The empty word gets no slot.
 * THE PARAMETERS.  marker: 0 to 4 bytes; when it is not empty it must be exactly one character by the rule below (for SentencePiece it
 * is U+2581 = E2 96 81).  unk_score: a finite float32 (SentencePiece's penalty is min(scores) - 10).  fuse_unk: 0 or 1.  max_bytes: in
 * 1 .. 4096.  seed: places the words in the tables and changes no id.
 * A TOKEN AND ITS MARKER.  A token is what latok_token_spans_utf8_bytes_batch yields: bytes [a, e) of string s.  A token is MARKED
 * when the marker is not empty, and the token is the first token of its string, or the previous token of the same string ends before
 * a, that is, whitespace was dropped in front of it.  A token that touches its predecessor is not marked: "hello," gives (marker)hello
 * and ",".
 * CHARACTERS AND POSITIONS.  A CHARACTER of a byte range starts at the range's first byte and at every later byte b with
 * (b & 0xC0) != 0x80; the rule is total on malformed bytes.  The VIRTUAL TEXT of a token is marker + bytes[a:e] when the token is
 * marked, else bytes[a:e].  Its POSITIONS 0 .. n are its character starts, plus its end.
 * THE CUT, per token:
 *   1. Long token.  If e - a > max_bytes, the token is ONE piece (unk_id, a, e).
 *   2. Forward pass.  Set best[0] = 0.0f; every other position is unset.  For i = 0 .. n-1 in ascending order, skipping an unset
 *      best[i]: for every position j > i whose virtual bytes [i, j) are a word w, compute cand = best[i] + score(w) -- ONE float32
 *      addition, nothing fused or reordered.  If best[j] is unset or cand > best[j] (strictly greater), then best[j] = cand and
 *      back[j] = (i, w).  If no word equals the single character [i, i+1), the same update is tried for j = i+1 with unk_score and
 *      w = unknown.  Every position ends up set.  Of equal scores the candidate met first stays, that is, the LOWER START and so the
 *      longer last piece.
 *   3. Backtrack.  Walk back from n through back.  A piece of virtual bytes [p, q) is reported with the string-relative byte range
 *      [max(p - m, 0) + a, (q - m) + a), where m is the marker's length for a marked token and 0 otherwise.  A piece that is the
 *      marker alone therefore has the empty range (a, a); a piece marker + prefix has range (a, a + len(prefix)).  An unknown piece
 *      emits unk_id.  With fuse_unk = 1, every maximal run of neighbouring unknown pieces of a token becomes ONE piece over the union
 *      of their ranges.  Runs never cross a token.
 *   4. Empty vocabulary.  V = 0 is accepted.  A token is then one unk piece (fused), or n unk pieces (not fused).
 * Exact as the ids call is: the hash finds the slot, the bytes decide.  This is the search of SentencePiece and of
 * tokenizers.models.Unigram (which adds in float64: with scores whose sums are exact in float32 the two agree).
 * latok_unigram_create takes HOST pointers and refuses, before any device work, what latok_vocab_create refuses, a non-finite score or
 * unk_score, a marker longer than 4 bytes or of more than one character, a fuse_unk outside 0 / 1 and a max_bytes outside 1 .. 4096.
 * The object holds two immutable tables of the kind latok_vocab holds (every word; the words behind the marker, without it; the slot
 * holds the word's position), an int32 array position -> id, a float32 array position -> score, the longest word and the
 * marker-alone word.  It may be used by any context of its device, concurrently; latok_unigram_destroy drains the current context
 * first, like latok_vocab_destroy.  latok_unigram_info reports the word count as given, the slots of the two tables, the longest word
 * of either table in bytes, the position of the marker-alone word (-1: none), the marker (4 bytes are written) and its length,
 * unk_score, fuse_unk, max_bytes, the seed and the device; any output pointer may be NULL.
 * The two calls have the contract of the BPE calls above, word for word: indptr / ids / spans as there, host pointers or
 * LATOK_DEVICE_PTRS, total_bytes = -1, the check of the object's device, LATOK_OUT_INT32 for indptr and spans, any other flag bit
 * refused before any device work; the capacity protocol in PIECES (cap too small: nothing is written to ids or spans, indptr stays
 * valid, the need is in *n_pieces_out, LATOK_ERR_INVALID; cap = 0 with ids_out = NULL is a size query; ids_out = NULL with cap > 0 is
 * refused); a batch with 2^31 pieces or more is refused; n_str = 0 or total_bytes = 0 as there.  The PADDED form writes the
 * [n_str, max_length] int32 block with bos_id / eos_id under add_special, and lengths_out.
 * Out of scope: SentencePiece's normalizer (NFKC, whitespace escaping) -- tokens are latok's, and folding is not part of these calls --,
 * byte_fallback, sampling / n-best, a .model protobuf loader, a flow form, an EOS-only padded layout (T5), a decoder mode that turns
 * the marker back into spaces (LATOK_DETOK_CONCAT gives the bytes with the marker in them), a prefix filter or trie in front of the
 * probes. */
typedef struct latok_unigram latok_unigram;
int latok_unigram_create(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                         const float* scores /* [n_words] */, const int32_t* word_ids /* may be NULL */, const uint8_t* marker,
                         int marker_len /* 0 .. 4 */, float unk_score, int fuse_unk, int max_bytes, uint32_t seed, latok_unigram** uni_out);
int latok_unigram_destroy(latok_unigram* uni);
int latok_unigram_info(const latok_unigram* uni, int64_t* n_words, int64_t* n_slots_plain, int64_t* n_slots_marked, int64_t* max_len,
                       int64_t* marker_word, uint8_t* marker_out /* [4] */, int* marker_len, float* unk_score, int* fuse_unk,
                       int* max_bytes, uint32_t* seed, int* device);
int latok_unigram_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                       const latok_unigram* uni, int32_t unk_id, int64_t* indptr_out /* [n_str+1] */, int32_t* ids_out,
                                       int64_t* spans_out /* may be NULL */, int64_t cap, int64_t* n_pieces_out,
                                       int64_t* n_tokens_out /* may be NULL */, int flags, void* stream);
int latok_unigram_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                          const latok_unigram* uni, int32_t unk_id, int64_t max_length, int add_special, int32_t bos_id,
                                          int32_t eos_id, int32_t pad_id, int32_t* input_ids_out /* [n_str*max_length] */,
                                          int32_t* lengths_out /* [n_str] */, int64_t* n_pieces_out /* may be NULL */, int flags,
                                          void* stream);

/* Decoding: ids back to UTF-8 bytes, for the ids of the encoder families above, whatever pre-tokenizer made them.
 * A DECODER is a device object of its own, built from a word list in the words / word_off layout latok_vocab_create takes (HOST
 * pointers) and an optional int32 array word_ids (NULL means id = index).  Every int32 is a legal id; of several words with one id the
 * LOWEST INDEX wins; the empty word is a legal entry and contributes no bytes; duplicate words with different ids are all kept (a
 * decoder maps ids, not words).  mode: LATOK_DETOK_CONCAT (BPE: tiktoken's decode_bytes) or LATOK_DETOK_WORDPIECE (the
 * " ".join(tokens).replace(" ##", "") rule of BERT tokenizers, with `prefix` of prefix_len = 0 .. 8 bytes and the separator byte `sep`
 * = 0 .. 255).  A word is a CONTINUATION word iff it starts with the prefix and is longer than the prefix.  The object holds the word
 * bytes in one blob below 2^32 bytes, one record per word and a map id -> word: a dense array over [min_id, max_id] when that range is
 * small against the word count (default ids, .tiktoken files, vocab.txt), else the sorted distinct ids, searched by bisection.
 * latok_detok_create refuses, before any device work, what latok_vocab_create refuses, a mode other than the two, a prefix_len outside
 * 0 .. 8, a sep outside 0 .. 255, and in CONCAT mode a prefix_len or sep other than 0.  The object may be used by any context of its
 * device, concurrently; latok_detok_destroy drains the current context first, like latok_vocab_destroy.  latok_detok_info reports the
 * word count as given, the distinct ids, the bytes of the blob, the longest word, the mode, whether the map is dense, and the device;
 * any output pointer may be NULL.
 * THE RULE.  A row is a sequence of ids.  A piece is DROPPED when its id is one of the n_skip = 0 .. 16 ids of skip_ids (a HOST pointer
 * in every mode: pad / BOS / EOS / [CLS] / [SEP]) or when its id is not in the object (unknown); a dropped piece leaves no trace in
 * its row.  Unknown pieces are counted in *n_unknown_out (may be NULL), skipped pieces are not.  The remaining pieces have words
 * w_0 .. w_k.  CONCAT: the row is w_0 + w_1 + .. + w_k.  WORDPIECE: w_0 verbatim, prefix included; for j >= 1 a continuation word
 * without its prefix, any other word as the sep byte followed by the word.  For a vocabulary in which no word contains the sep byte
 * and the bare prefix is not a word this equals sep.join(words).replace(sep + prefix, b"").  Bytes out: nothing looks at UTF-8
 * structure; the caller decodes.
 * latok_detok_csr takes the rows as a CSR: indptr [n_rows + 1] (int64, or int32 under LATOK_OUT_INT32; out_off is int64 in every mode)
 * and n_pieces ids, validated as latok_tfidf_csr validates its CSR -- a refused call writes nothing.  latok_detok_padded takes the
 * [n_rows, max_length] block of the padded encoder calls: row s is the first lengths[s] cells of row s of the block; lengths == NULL
 * means all max_length cells (put pad_id into skip_ids); a length outside [0, max_length] refuses the call.  Host pointers, or
 * LATOK_DEVICE_PTRS for ids, indptr, lengths and the outputs; any other flag bit is refused before any device work; the object's
 * device is checked as in the calls above.  Output: out_bytes, the rows' bytes back to back, and out_off [n_rows + 1], row s =
 * out_bytes[out_off[s] : out_off[s + 1]].  The capacity protocol in BYTES is latok_fold_utf8_bytes_batch's: out_cap too small: nothing
 * is written to out_bytes, out_off stays valid, the need is in *n_out_bytes, LATOK_ERR_INVALID; out_cap = 0 with out_bytes = NULL is a
 * size query; out_bytes = NULL with out_cap > 0 is refused.  n_rows = 0 or no pieces: zero bytes, out_off cleared.  Blocking: one wait
 * for the totals, one more behind the copies with host pointers.  Every batch size takes the same kernels.  The output of a device
 * call is a valid utf8 / byte_off input of every byte-space call when its start is 16-byte aligned.
 * Out of scope: a flow form, decoding to text with error replacement, special-token strings beyond what the vocabulary holds as
 * words.  (The ids of a Unigram model decode in CONCAT mode with a decoder built from the same word list: the marker stays in the bytes.) */
#define LATOK_DETOK_CONCAT 0      /* BPE: a row is the concatenation of its words */
#define LATOK_DETOK_WORDPIECE 1   /* continuation words lose the prefix, other words get a separator in front */
typedef struct latok_detok latok_detok;
int latok_detok_create(const uint8_t* words, const int64_t* word_off /* [n_words+1], host */, int64_t n_words,
                       const int32_t* word_ids /* may be NULL: id = index */, int mode, const uint8_t* prefix, int prefix_len /* 0 .. 8 */,
                       int sep /* 0 .. 255 */, latok_detok** out);
int latok_detok_destroy(latok_detok* d);
int latok_detok_info(const latok_detok* d, int64_t* n_words, int64_t* n_ids, int64_t* blob_bytes, int64_t* max_len, int* mode, int* dense,
                     int* device);
int latok_detok_csr(const latok_detok* d, const void* indptr /* [n_rows+1] */, const int32_t* ids, int64_t n_rows, int64_t n_pieces,
                    const int32_t* skip_ids, int n_skip, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off /* [n_rows+1] */,
                    int64_t* n_out_bytes, int64_t* n_unknown_out /* may be NULL */, int flags, void* stream);
int latok_detok_padded(const latok_detok* d, const int32_t* input_ids /* [n_rows*max_length] */, const int32_t* lengths /* [n_rows], may be NULL */,
                       int64_t n_rows, int64_t max_length, const int32_t* skip_ids, int n_skip, uint8_t* out_bytes, int64_t out_cap,
                       int64_t* out_off, int64_t* n_out_bytes, int64_t* n_unknown_out, int flags, void* stream);

/* Case folding and accent stripping in byte space: UTF-8 in, folded UTF-8 out, what an uncased vocabulary (bert-base-uncased and its
 * relatives) or a lower-casing vectorizer needs in front of the token calls above.  `fold` is a set of LATOK_FOLD_* bits in an
 * argument of its own; any other bit is refused before any device work.
 * THE MAP F_fold(c) takes one code point to 0 .. 3 code points; nothing depends on neighbouring characters.  Its data is Python's
 * str.lower() and unicodedata of the interpreter that built the library; latok_amd/csrc/fold_tables.inc, generated by the build,
 * records the UCD version in its first line (13.0.0 under Python 3.10, which is what the tests' fixture holds).
 *   1. CLEAN (the _clean_text rule of BERT): c == 0, c == U+FFFD, or a category in {Cc, Cf} other than U+0009 / U+000A / U+000D maps to
 *      the empty sequence; U+0009, U+000A, U+000D, U+0020 and category Zs map to [U+0020]; in both cases the map is done.
 *   2. seq = [c].  LOWER: seq = the code points of chr(c).lower() (U+0130 gives two; no final-sigma rule: U+03A3 always gives
 *      U+03C3).  STRIP_MARKS: every x of seq is replaced by the code points of its canonical decomposition (NFD) whose category is
 *      not Mn; Hangul syllables become 2 .. 3 jamo by the arithmetic rule, the Mn code points map to nothing.
 *   3. CJK_SPACE: c in 4E00-9FFF, 3400-4DBF, 20000-2A6DF, 2A700-2B73F, 2B740-2B81F, 2B820-2CEAF, F900-FAFF or 2F800-2FA1F gives
 *      [U+0020] + seq + [U+0020].
 *   4. Surrogates D800-DFFF and values above 0x10FFFF are their own image.
 * The longest image has 3 code points and 12 bytes; the largest growth in bytes is 3x (a Hangul LVT syllable: 3 -> 9, U+1D160: 4 ->
 * 12), the smallest image is empty.  So out_off[n_str] <= 3 * total_bytes: size buffers by it.
 * THE BYTE RULE: the result for string s depends on the bytes of string s alone.  With k(b0) = 0 below 0x80 and for 0x80 .. 0xBF, 1
 * for 0xC0 .. 0xDF, 2 for 0xE0 .. 0xEF, 3 for 0xF0 .. 0xFF, a byte b0 at i with k(b0) > 0 opens a SEQUENCE iff bytes i+1 .. i+k lie
 * inside the same string and are all 10xxxxxx; a byte below 0x80 is a sequence of its own.  The sequence's value c is its payload
 * bits put together (overlong, surrogate and too-large forms decode as they are; 0xF8 .. 0xFF carry 3 payload bits).  A sequence with
 * F_fold(c) == [c] is copied verbatim, source bytes unchanged -- overlong forms survive --; any other sequence is replaced by the
 * shortest-form UTF-8 of its image.  Every byte that belongs to no sequence (a lead with a truncated tail, a stray continuation
 * byte) is copied verbatim: it is never taken for U+FFFD, and CLEAN does not drop it.  fold == 0 is the identity copy.  Nothing is
 * invented and nothing is lost on malformed bytes, and for well-formed text t the output is "".join(F_fold(c) for c in t) in UTF-8.
 * Relation to BERT: for text without U+03A3 and without the 23 code points that are not Mn and have a nonzero combining class,
 * LOWER | STRIP_MARKS equals "".join(ch for ch in NFD(t.lower()) if category(ch) != "Mn"); the differences are the final sigma and
 * the canonical reordering of surviving marks.
 *   out_off[0] = 0, out_off[s+1] = out_off[s] + len(fold(string s)),  out_bytes[out_off[s] : out_off[s+1]] = fold(string s)
 * Capacity protocol, in BYTES: out_cap too small -> nothing is written to out_bytes, out_off stays valid, the needed size is in
 * *n_out_bytes and the call returns LATOK_ERR_INVALID; out_cap = 0 with out_bytes = NULL is a size query; out_bytes = NULL with
 * out_cap > 0 is refused.  Host pointers or LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned; the output then starts wherever
 * the caller says and is a valid input of every byte-space call if that is 16-byte aligned), total_bytes = -1 as in the sibling
 * calls; any other flag bit is refused.  n_str = 0 or total_bytes = 0 gives zero bytes with out_off cleared.  With device pointers the
 * call synchronises once; with host pointers a second time behind the copy of the bytes.  Every batch size takes the same kernels and
 * gives the same bytes.  Run-time rule tables (latok_set_rules) have no bearing on it.  The tables of the map reach the device with
 * the first fold call of a context, not in latok_init. */
#define LATOK_FOLD_LOWER 1
#define LATOK_FOLD_STRIP_MARKS 2
#define LATOK_FOLD_CLEAN 4
#define LATOK_FOLD_CJK_SPACE 8
int latok_fold_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int fold,
                                uint8_t* out_bytes, int64_t out_cap, int64_t* out_off /* int64[n_str+1] */,
                                int64_t* n_out_bytes, int flags, void* stream);

/* Token counting in byte space: the vocabulary of a corpus -- every distinct token with its frequency -- built on the device.
 * The tokens of a batch are the byte slices latok_token_spans_utf8_bytes_batch reports for it (default_tokenizer.py:149-160);
 * run-time rule tables and malformed bytes are taken as that call takes them, and bytes are compared verbatim.  A COUNTER is a
 * mutable device object with three fixed properties: max_word_bytes in 1 .. 256 (another value is refused before any device work;
 * there is no form for longer words), a table of n_slots = a power of two >= 2 max_words and >= 64 (max_words in 1 .. 2^30), and
 * a 32-bit seed (of the MurmurHash3 x86_32 that places a word; it changes no count).  After any sequence of updates:
 *   count[w]  = number of tokens equal to w, byte for byte, over all updates, for every word w the counter holds
 *   tokens    = counted + long + dropped, always
 *   long      = tokens of more than max_word_bytes bytes: tallied, never entered
 *   dropped   = tokens that found neither their word nor a free slot within the probe bound (128 slots, or n_slots if smaller)
 *   distinct  = words held
 * dropped = 0 means the counter holds exactly the distinct tokens of at most max_word_bytes bytes, with exact counts; at
 * most max_words distinct words in a table of 2 max_words slots drop only if 128 occupied slots lie in a row, which at that load
 * has a probability of about 1e-11 per slot: not in practice, but it is the stats that say so, not the sizing.  dropped > 0 means every held count is a lower bound and
 * no held word is missing from the text.  Exact as the ids call is: the hash finds the slot, the bytes decide.  The order in which
 * latok_counter_read lists the words is unspecified (it depends on which thread wins a slot); everything else is deterministic.
 * latok_counter_create makes an empty counter on the device of the current context.  latok_counter_info needs no device; any
 * output pointer may be NULL; stats5 = {tokens, counted, long, dropped, distinct}, totals over all updates.  latok_counter_clear
 * empties the counter.  latok_counter_destroy drains the current context (its stream and its flow) first, like latok_vocab_destroy, and
 * frees the counter whatever the drain reports.
 * The update call follows latok_token_ids_utf8_bytes_batch in everything that is not the counting: host pointers or
 * LATOK_DEVICE_PTRS (device UTF-8 pointer 16-byte aligned), total_bytes = -1 accepted; any other flag bit, LATOK_OUT_INT32 included,
 * is refused before any device work, and so are a NULL counter, a counter on another device than the current context's, a counter
 * in the failed state and a batch of 2^39 bytes or more.  n_str = 0 or total_bytes = 0 leaves the counter untouched and zeroes
 * stats4_out = {tokens, counted, long, dropped} of THIS call (may be NULL).  Every batch size takes the same kernels.  When the call
 * returns, the counter holds copies of its words: the caller's text may be overwritten or freed.
 * Calls on one counter are serialised by a lock inside it; two contexts of one device may share it.  The object is NOT immutable,
 * so there is no flow form: two batches in flight would race on the table's state.
 * FAILED STATE: if an update fails after its counting kernel was enqueued and before its words were copied (a HIP error, no memory
 * for the words), the counter is marked failed: every later call on it except latok_counter_clear and latok_counter_destroy
 * returns LATOK_ERR_INVALID.
 * latok_counter_read takes HOST pointers and the capacity protocol of the siblings: cap = 0, bytes_cap = 0 with NULL buffers is a
 * size query; if either capacity is too small nothing is written but *n_words_out and *n_bytes_out, and the call returns
 * LATOK_ERR_INVALID.  words_out / word_off_out have exactly the layout latok_vocab_create takes (the words back to back,
 * word_off_out[n_words + 1] from 0), counts_out[i] is the count of word i. */
typedef struct latok_counter latok_counter;
int latok_counter_create(int64_t max_words, int max_word_bytes, uint32_t seed, latok_counter** out);
int latok_counter_destroy(latok_counter* counter);
int latok_counter_clear(latok_counter* counter);
int latok_counter_info(const latok_counter* counter, int64_t* max_words, int64_t* n_slots, int* max_word_bytes, uint32_t* seed,
                       int* device, int64_t* stats5);
int latok_count_tokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                        latok_counter* counter, int64_t* stats4_out /* may be NULL */, int flags, void* stream);
int latok_counter_read(const latok_counter* counter, uint8_t* words_out, int64_t bytes_cap, int64_t* word_off_out /* [cap+1] */,
                       uint64_t* counts_out, int64_t cap, int64_t* n_words_out, int64_t* n_bytes_out);

/* Token feature vectors: reference featurize() (default_tokenizer.py:163-191) for a whole batch without the n x 25
 * matrix.  Per kept token k: spans4_out[4k..4k+3] = {raw_start, raw_end, strip_start, strip_end} (LaToken.start_idx /
 * end_idx are the raw span, LaToken.text is text[strip_start:strip_end]); features_out[25k..25k+24] = sum of the 25
 * feature columns over the raw span in uint8 wrap-around arithmetic (latok.c:342-354).  cap in tokens. */
int latok_token_features_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                               int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                               int64_t* n_tokens_out, int flags, void* stream);

/* ---- PEP 393 buffers: the reference's own input format ------------------------------------------------------------
 * The reference reads a str through PyUnicode_KIND / PyUnicode_DATA (latok.c:53-55,79): fixed-width code units of
 * kind = 1 (Latin-1), 2 (UCS-2) or 4 (UCS-4) bytes.  These entry points take that buffer as it is: `units` = the
 * packed units of all strings, row_off / total_chars / every result in units = chars (CPython stores text with astral
 * chars as kind 4, so a kind-2 unit is always a whole code point; lone surrogates are classified as the code points
 * they are).  A caller that holds Python strings never widens them to UTF-32, and a Latin-1 / UCS-2 batch costs 1 / 2
 * bytes per char on the bus and in HBM: the tile kernel reads the narrow units itself (mask, offsets, spans), under
 * run-time rule tables as well; only featurize widens them once on the device (it re-reads the code points).  Results
 * are identical to the UTF-32 entry points on the widened text.  kind = 4 forwards to those.  With LATOK_DEVICE_PTRS `units` must be 16-byte aligned. */
int latok_split_mask_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                uint64_t* mask_bits_out, int flags, void* stream);
int latok_split_offsets_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                   int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap, int64_t* n_offsets_out,
                                   int flags, void* stream);
int latok_token_spans_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                 int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                 int flags, void* stream);
int latok_token_features_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                    int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                    int64_t* n_tokens_out, int flags, void* stream);

/* ---- the reference's three native functions, one string at a time (compat surface) ---------------------------- */
/* _gen_parse_matrix (latok.c:31-138): n code points -> int8[n][25], C-contiguous. */
int latok_parse_matrix(const uint32_t* cps, int64_t n, int8_t* matrix_out, int flags, void* stream);

/* _combine_matrix_rows (latok.c:275-370): m is a 2-D byte matrix addressed m[r*stride_r + c*stride_c] with `rows`
 * rows and `cols` columns; idx is int8, idx_ndim 2 (irows x icols, "sum of products", -1 skipped) or 1 (icols row
 * ids, "sum").  out = int8[cols].  uint8 wrap-around arithmetic like the reference.  The matrix is copied densely
 * (rows x cols) before upload when given as host pointers; in device mode strides are honoured as given. */
int latok_combine_matrix_rows(const int8_t* m, int64_t rows, int64_t cols, int64_t stride_r, int64_t stride_c,
                              const int8_t* idx, int idx_ndim, int irows, int icols, int8_t* out, int flags,
                              void* stream);

/* _gen_block_mask (latok.c:140-258): a1 ("starts") and a2 ("spaces") are int8[n], non-zero = set. out = int8[n]. */
int latok_block_mask(const int8_t* a1, const int8_t* a2, int64_t n, int8_t* out, int flags, void* stream);

/* ---- device memory / stream helpers (so hosts need no other GPU runtime binding) ------------------------------ */
void* latok_dev_alloc(size_t bytes);   /* NULL on failure */
int latok_dev_free(void* p);
/* Pinned (page-locked) host memory: host-pointer batches handed over in such buffers move over the bus at full speed and
 * asynchronously -- the chunked pipeline of the large-batch compaction calls then keeps both copy directions busy at once. */
void* latok_host_alloc(size_t bytes);  /* NULL on failure */
int latok_host_free(void* p);
int latok_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);
int latok_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
int latok_memset_dev(void* dst_dev, int value, size_t bytes);
int latok_sync(void);                  /* wait for the library stream */
int latok_device_props(int* n_cu, int64_t* hbm_bytes, char* name_out, int name_cap);

/* ---- synthetic corpora (counter-based, identical on host and device) ------------------------------ */
#define LATOK_CORPUS_ASCII 0
#define LATOK_CORPUS_UNICODE 1
/* row_off_out[n_str + 1] (host): lengths uniform in [len_lo, len_hi] for string ids sid0 .. sid0+n_str-1 */
int latok_corpus_offsets(uint64_t seed, uint64_t sid0, int64_t n_str, int64_t len_lo, int64_t len_hi,
                         int64_t* row_off_out);
/* fill code points; host form (pure CPU, no device needed) and device form (one thread per string) */
int latok_corpus_fill_host(uint64_t seed, int model, uint64_t sid0, int64_t n_str, const int64_t* row_off,
                           uint32_t* cps_out);
int latok_corpus_fill_device(uint64_t seed, int model, uint64_t sid0, int64_t n_str, const int64_t* row_off_dev,
                             uint32_t* cps_out_dev, void* stream);
/* total UTF-8 encoded size of n code points (device pointers when LATOK_DEVICE_PTRS); result to a host int64 */
int latok_utf8_bytes(const uint32_t* cps, int64_t n, int64_t* bytes_out, int flags);

/* ---- runtime rule tables ------------------------------------------------------------------------------------------
 * The reference's extension point (latok/core/default_tokenizer.py:9-30,108-110): other C_SPLIT / C_MASK / C_SYM
 * matrices built with build_combo_matrix (latok/core/latok_utils.py:27-56) over the 25 feature columns
 * (latok/core/offsets.py:24-49), combined as gen_split_mask does (default_tokenizer.py:113-134):
 *     splits = combine(C_SPLIT) * block_mask(combine(C_MASK), SPACE) + combine(C_SYM);  splits[0] = 1
 * with combine = _combine_matrix_rows (latok.c:275-370).  After latok_set_rules EVERY batch entry point evaluates the
 * caller's tables inside the fused kernel, for every input form -- UTF-32, UTF-8 in byte space, UTF-8 in code-point
 * units, PEP 393 kind 1 / 2 units (each has its own tile-kernel instantiation; nothing is widened or decoded first) --
 * and every output: bitmask, offsets, token spans, featurize, and latok_split_values_batch, which then returns what
 * gen_split_mask returns for those tables: (number of C_SPLIT rows that hold) * mask + (number of C_SYM rows that hold),
 * 1 at a string start.  Boundaries and values are bit-exact with the reference recipe run on the same tables.  Each
 * table is a row-major int8 [rows x cols] matrix of column ids, -1 padding short rows; limits: <= 32 rows per table (the
 * rows travel in the kernel arguments; the reference's own tables have 5 / 4 / 1), ids 0..24, a row must not START
 * with -1 (the reference would reuse the previous row's product there).  rows = 0 gives the all-zero vector.  State of
 * the current context. */
int latok_set_rules(const int8_t* c_split, int split_rows, int split_cols, const int8_t* c_mask, int mask_rows,
                    int mask_cols, const int8_t* c_sym, int sym_rows, int sym_cols);
int latok_reset_rules(void);   /* back to the built-in default_tokenizer.py tables */
int latok_rules_active(void);  /* 1 while custom tables are installed */

/* ---- batch flow: many device-resident batches through one context, overlapped -------------------------------------------
 * The reference tokenizes one string after another (default_tokenizer.py:137-160: every call is independent of the one
 * before).  Here a batch costs three dependent launches (per-tile string index, tiles, resolve); only the tile kernel needs
 * the whole GPU.  A flow keeps up to TWO batches in flight on the current context -- every batch in flight on a stream and
 * a workspace set of its own (a "slot"; submissions take the slots in turn), with no dependency between the slots -- so that
 * the two small launches of one batch run beside the tile kernel of the other; a flow batch's tile kernel is planned for 7/8 of
 * the CUs, so consecutive tile kernels overlap their start-up and ragged end as well (C2: 0.108 -> 0.087 ms per batch).
 *   latok_flow_split_mask: enqueue latok_split_mask_batch(LATOK_DEVICE_PTRS) of one batch and return.  The inputs must be
 *     complete in device memory when the call is made (they are NOT ordered behind work on any caller stream), and must stay
 *     untouched by the caller until latok_flow_wait.  total_chars < 0: read from row_off (one small synchronous copy).
 *     Results are bit-identical to latok_split_mask_batch.
 *   latok_flow_wait: block until every batch submitted on the current context is complete (latok_sync does the same).  The
 *     streams are polled for up to 2 ms before the call sleeps on them (a sleeping wait returns ~15 us late).
 * Ordering between batches of one flow.  Every call is independent, as the reference's calls are -- batches that touch
 * disjoint memory overlap freely.  The library tracks the byte RANGE of every buffer a batch in flight reads (units, row
 * offsets) or writes (mask; for the compaction calls: records, counts, result words, feature sums; for the code-point UTF-8
 * calls at the end of this section also the code-point row offsets and all four result words) until the flow is next idle.  A new batch that writes any byte a batch still in flight reads or writes, or reads one it writes -- whole buffer or
 * partial overlap, however many other batches were submitted in between -- is ordered behind that batch (it is enqueued on that
 * batch's slot; if batches on both slots are in its way the call first waits for the flow to drain).  So reusing an output
 * buffer is always correct, it just does not overlap; callers that want the overlap alternate their buffers.
 * The blocking entry points may be called on the same context while a flow is in flight (they use the context's own stream
 * and workspace; their buffers are NOT tracked against the flow's).  A batch larger than any its slot has seen grows the
 * slot's workspace, which first waits for the flow to drain. */
int latok_flow_split_mask(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                          uint64_t* mask_dev);
/* The same for the other input forms of the path: PEP 393 units (kind 1 / 2 / 4 as latok_split_mask_kind_batch; positions are
 * chars) and UTF-8 in byte space (as latok_split_mask_utf8_bytes_batch; positions are bytes).  Batches of different forms may
 * follow each other in one flow. */
int latok_flow_split_mask_kind(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                               uint64_t* mask_dev);
int latok_flow_split_mask_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                     uint64_t* mask_dev);
/* Boundary offsets / token spans of a batch through the flow: what latok_split_offsets_batch / latok_token_spans_batch (and
 * their _kind / _utf8_bytes forms) compute, enqueued without waiting for the item total.  kind: 4 = UTF-32 code points, 1 / 2 =
 * PEP 393 units, 0 = UTF-8 bytes in byte space (row_off = byte offsets, positions are bytes).  Every pointer is a device
 * address (LATOK_DEVICE_PTRS is implied); flags: LATOK_OUT_INT32 for int32 counts / records.
 *   counts_dev[n_str], offsets_dev[offsets_cap] (spans_dev[2 * spans_cap]): as in the blocking calls.
 *   result_dev: int64[2] in memory the DEVICE can write and the caller can read after latok_flow_wait (latok_dev_alloc +
 *     latok_memcpy_d2h, or latok_host_alloc for a direct read): result[0] = number of items of the batch, result[1] = 0, or
 *     nonzero when the batch could not be reported (low half: a string of >= 2^31 chars under LATOK_OUT_INT32; high half:
 *     internal scan error, the call is safe to repeat).  When result[0] exceeds the capacity nothing was written to the
 *     records (counts are valid): resubmit with a larger buffer -- the capacity protocol of the blocking calls, read late.
 * Every output (records, counts, result words) takes part in the ordering rule above. */
int latok_flow_split_offsets(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_units,
                             void* counts_dev, void* offsets_dev, int64_t offsets_cap, int64_t* result_dev, int flags);
int latok_flow_token_spans(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_units,
                           void* counts_dev, void* spans_dev, int64_t spans_cap, int64_t* result_dev, int flags);
/* featurize through the flow: latok_token_features_batch / _kind_batch (kind 4 / 1 / 2) with the same result words */
int latok_flow_token_features(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                              void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev, int flags);
/* UTF-8 in CODE-POINT units through the flow: what latok_split_mask_utf8_batch, latok_split_offsets_utf8_batch,
 * latok_token_spans_utf8_batch and latok_token_features_utf8_batch report for the same batch (positions are code points of
 * the decoded text, as the reference reports them), bit-identical, enqueued without waiting for anything: the code-point total
 * stays on the device, where the stages behind the lead-byte scan read it.  Every pointer is a device address; utf8_dev
 * 16-byte aligned; total_bytes < 0: read from byte_off (one small synchronous copy); batches of every size take this route.
 *   result_dev: int64[4], 8-byte aligned, device-writable, read after latok_flow_wait:
 *     result[0]  number of items (offsets / tokens); 0 for the mask form
 *     result[1]  as above: low half = a string of >= 2^31 chars under LATOK_OUT_INT32, high half = the chained scan did
 *                not complete (safe to repeat)
 *     result[2]  code-point total of the batch (total_cps_out of the blocking call)
 *     result[3]  nonzero = the batch holds MALFORMED UTF-8 that the byte-space model and the staged decoder read differently
 *                (a continuation byte without a lead byte in the 3 bytes before it, or at the start of a string).  Then NO
 *                record, count, mask word or row offset of this batch is valid (records and feature sums are not written at
 *                all): resubmit the batch through the blocking _utf8_batch call, which has the staged decoder.  The flow
 *                reports such input; it does not decode it.
 *   Capacity: when result[0] exceeds the capacity no record is written and counts are valid.  Mask form: mask_dev holds
 *     mask_cap_words words; ceil(total_bytes / 64) always suffice; when ceil(result[2] / 64) exceeds mask_cap_words no mask
 *     word is written (row offsets are).  Bits of the last meaningful word above the total are zero.  cp_row_off_dev[n_str + 1].
 *   n_str == 0 or total_bytes == 0: the result words, counts and row offsets are cleared on the slot's stream.
 * The four result words, mask, row offsets, counts, records, feature sums and the inputs take part in the ordering rule. */
int latok_flow_split_mask_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                               uint64_t* mask_dev, int64_t mask_cap_words, int64_t* cp_row_off_dev, int64_t* result_dev);
int latok_flow_split_offsets_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                  void* counts_dev, void* offsets_dev, int64_t offsets_cap, int64_t* result_dev, int flags);
int latok_flow_token_spans_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                void* counts_dev, void* spans_dev, int64_t spans_cap, int64_t* result_dev, int flags);
int latok_flow_token_features_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                   void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap,
                                   int64_t* result_dev, int flags);
/* featurize in BYTE space through the flow: what latok_token_features_utf8_bytes_batch reports (span records in byte positions,
 * sums per char), bit-identical, with the conventions of latok_flow_token_features_utf8: the same four result words (result[2] =
 * code-point total; result[3] nonzero = malformed UTF-8: no record and no sum was written -- the blocking call refuses the same
 * batch), the same capacity rule, every buffer in the ordering rule; under LATOK_OUT_INT32 a string of 2^31 BYTES sets result[1]. */
int latok_flow_token_features_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                         void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap,
                                         int64_t* result_dev /* int64[4] */, int flags);
/* Joined token text through the flow: what latok_join_tokens_utf8_bytes_batch reports (sep.join of every string's tokens,
 * reference default_tokenizer.py:149-160; the definition is at that call), byte-identical, without waiting: result[0] = output
 * bytes (= out_off[n_str]), result[1] = error word -- bit 0: a string too long for LATOK_OUT_INT32 counts, bit 2 (value 4): the
 * batch needs more than out_cap bytes (nothing was written to out_bytes; out_off, counts and result[0] are valid), upper half: the
 * scan's internal flag.  Read them after latok_flow_wait.  counts_dev may be NULL.  The ordering rule covers the input bytes,
 * byte_off, out_bytes (min(out_cap, 2 * total_bytes) bytes of it), out_off, counts and the result words. */
int latok_flow_join_tokens_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                      int sep, uint8_t* out_bytes_dev, int64_t out_cap, int64_t* out_off_dev,
                                      void* counts_dev, int64_t* result_dev /* int64[2]: output bytes, error word */, int flags);
/* Token hashes through the flow: what latok_token_hashes_utf8_bytes_batch reports (MurmurHash3 x86_32 of every token of
 * default_tokenizer.py:149-160; the definition is at that call), word for word, without waiting.  The two result words of
 * latok_flow_token_spans: result[0] = tokens, result[1] = error word (bit 0: a string too long for LATOK_OUT_INT32, upper half:
 * the scan's internal flag), and its capacity rule, read late: result[0] > cap means nothing was written to hashes or records
 * (counts are valid).  Read them after latok_flow_wait.  counts_dev and spans_dev may be NULL.  The ordering rule covers the
 * input bytes, byte_off, hashes and records (min(cap, total_bytes) tokens of each), counts and the result words. */
int latok_flow_token_hashes_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                       uint32_t seed, void* counts_dev, void* spans_dev, uint32_t* hashes_dev, int64_t cap,
                                       int64_t* result_dev /* int64[2]: tokens, error word */, int flags);
/* Token ids through the flow: what latok_token_ids_utf8_bytes_batch reports (the id of every token of default_tokenizer.py:149-160
 * in `vocab`, unk_id where it has none; the definition is at that call), id for id, without waiting.  The two result words and the
 * late-read capacity rule of latok_flow_token_hashes_utf8_bytes: result[0] = tokens, result[1] = error word; result[0] > cap means
 * nothing was written to ids or records (counts are valid).  Read them after latok_flow_wait.  counts_dev and spans_dev may be
 * NULL.  The ordering rule covers the input bytes, byte_off, ids and records (min(cap, total_bytes) tokens of each), counts and
 * the result words; the vocabulary's table is library-owned read-only memory and takes no part in it. */
int latok_flow_token_ids_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                    const latok_vocab* vocab, int32_t unk_id, void* counts_dev, void* spans_dev,
                                    int32_t* ids_dev, int64_t cap, int64_t* result_dev /* int64[2]: tokens, error word */, int flags);
int latok_flow_wait(void);

/* ---- measurement ----------------------------------------------------------------------------------------------- */
/* Run latok_split_mask_batch on device-resident data: `warmup` untimed passes, then
 *   ms_total_out  = elapsed ms of `iters` whole-pipeline passes (tile index, tiles, resolve) between ONE pair of HIP events
 *                   on the stream the kernels run on;
 *   ms_tiles_out  = elapsed ms of `iters` further launches of the dominant kernel alone (k_tiles_main, back to back,
 *                   again one event pair: an event pair per launch charges each interval with ~6 us of marker dispatch);
 *   n_fix_tiles_out = tiles recomputed by the resolve stage in the last pass.
 * Any may be NULL (a NULL output skips its passes), so warm-up-only and kernel-only calls are possible. */
int latok_bench_split_mask(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                           uint64_t* mask_dev, int warmup, int iters, float* ms_total_out, float* ms_tiles_out,
                           int64_t* n_fix_tiles_out);

/* Streaming-read ceiling of this GPU: time `iters` launches of a kernel that only reads `bytes` (a multiple of 16 KiB
 * is used; device pointer, 16-byte aligned) with the tile kernel's load pattern.  ms_out = elapsed ms of the `iters`
 * launches after `warmup` untimed ones.  Measurement aid for SURVEY.md 8(d) ("vs. a measured streaming-read kernel"). */
int latok_bench_stream_read(const void* buf_dev, int64_t bytes, int warmup, int iters, float* ms_out);

/* Several contexts in one process, timed as ONE job (one host thread + one context per GPU, no collective).
 * A gate is a rendezvous of `parties` host threads that lives outside any context (no device needed):
 * latok_gate_wait returns on every thread once all of them have arrived (it spins inside the library, so a ctypes
 * caller has released the GIL) and fails with LATOK_ERR_INVALID after `timeout_s` seconds without the full set.  A gate
 * can be passed any number of times.  latok_gate_break makes every present and future wait fail at once (a party that
 * cannot reach the gate calls it so that the others do not sit out the timeout).
 * latok_bench_split_mask_gated = the timed region of the whole-job measurement on the CURRENT context:
 *   wait at `gate` (NULL: no wait) -> host clock t0 -> HIP event -> `iters` whole-pipeline passes -> HIP event ->
 *   stream synchronise -> host clock t1 -> wait at `gate` again (so that no thread starts anything else on the node while
 *   another is still inside its region).
 * ms_events_out = the event pair; t0_ns_out / t1_ns_out = the host's monotonic clock (one clock for every thread of the
 * process), so the job took max(t1) - min(t0) over the contexts. */
typedef struct latok_gate latok_gate;
int latok_gate_create(int parties, latok_gate** gate_out);
int latok_gate_destroy(latok_gate* gate);
/* The same rendezvous for one PROCESS per GPU: the gate lives in POSIX shared memory under `name` ("/something").  One
 * process creates it, the others attach; every process detaches when done and one of them unlinks the name.  The host's
 * monotonic clock is one clock for all processes of the machine, so t0 / t1 of latok_bench_split_mask_gated compare. */
int latok_gate_create_shared(const char* name, int parties, latok_gate** gate_out);
int latok_gate_attach_shared(const char* name, latok_gate** gate_out);
int latok_gate_detach_shared(latok_gate* gate);
int latok_gate_unlink_shared(const char* name);
int latok_gate_wait(latok_gate* gate, double timeout_s);
int latok_gate_break(latok_gate* gate);
int latok_bench_split_mask_gated(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                                 uint64_t* mask_dev, int iters, latok_gate* gate, float* ms_events_out,
                                 int64_t* t0_ns_out, int64_t* t1_ns_out);
/* The same timed region through the batch flow: `iters` latok_flow_split_mask submissions of the batch, writing mask_a_dev
 * and mask_b_dev alternately (two buffers of ceil(total_chars / 64) words), then latok_flow_wait -- every pass does all
 * three launches and completes inside the region.  ms_events_out: from an event in front of the first string-index launch
 * to one behind the last resolve launch. */
int latok_bench_split_mask_flow_gated(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                                      uint64_t* mask_a_dev, uint64_t* mask_b_dev, int iters, latok_gate* gate,
                                      float* ms_events_out, int64_t* t0_ns_out, int64_t* t1_ns_out);

/* A second, equal copy of the batch at another address for the two flow measurements (this one and latok_bench_tiles_flow): the
 * odd steps then read cps_b_dev / row_off_b_dev instead, so that the two batches in flight share no input lines in L2 / MALL -- as
 * two different batches of a real flow would not.  NULL, NULL: back to one shared input.  State of the current context. */
int latok_bench_set_second_input(const uint32_t* cps_b_dev, const int64_t* row_off_b_dev);

/* The dominant kernel alone in the flow's launch scheme: `iters` launches of k_tiles_main (planned for 7/8 of the CUs, as every
 * batch of a flow is) alternating between the two slot streams, nothing else launched; ms_out = host wall time from the first
 * launch to the end of the last (streams polled).  The launches overlap, so ms_out / iters is the kernel's average cost per
 * launch in the flow, not the duration of one launch. */
int latok_bench_tiles_flow(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                           uint64_t* mask_a_dev, uint64_t* mask_b_dev, int iters, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif
