/*
 * femto_amd.h -- C ABI of the MI355X-native FM-index query engine (drop-in for femto's batched
 * count/locate path).  Plain pointers and sizes only; no C++/torch/HIP types in any signature.
 *
 * The reference (femto-dev/femto v1.3.0) exposes no plugin ABI; its batch entry points are the C
 * functions of src/main/femto_internal.h.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference tree).  INTEGRATION.md shows the shim a femto
 * maintainer would add so that parallel_count()/parallel_locate() call into this library.
 *
 * Conventions kept from the reference:
 *   - patterns are arrays of alpha_t (uint16_t) = byte + 5 (src/main/index_types.h:61-69);
 *   - every function returns an err_code_t value (src/utils/error.h:25-39), 0 = OK;
 *   - calls are blocking; a handle may be used from several host threads at once (every call leases a
 *     scratch and a stream of its own from the handle: concurrent calls overlap on the GPU);
 *   - results are bit-exact with parallel_count / parallel_locate on the same index files.
 *
 * All compute runs in hand-written HIP kernels on the GPU; there is NO CPU fallback: if no HIP
 * device is usable, femto_amd_open fails with FEMTO_AMD_ERR_INVALID.
 */
#ifndef FEMTO_AMD_H
#define FEMTO_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* err_code_t of src/utils/error.h:25-39 (same numeric values) */
enum {
  FEMTO_AMD_OK = 0,
  FEMTO_AMD_ERR_MEM = 1,
  FEMTO_AMD_ERR_IO = 2,
  FEMTO_AMD_ERR_PARAM = 3,
  FEMTO_AMD_ERR_FORMAT = 4,
  FEMTO_AMD_ERR_BZ_DATA = 5,
  FEMTO_AMD_ERR_INVALID = 6,
  FEMTO_AMD_ERR_MISSING = 8,
  FEMTO_AMD_ERR_FULL = 10,
  FEMTO_AMD_ERR_OVERWORKED = 11,
  FEMTO_AMD_ERR_UNKNOWN = 12
};

#define FEMTO_AMD_ALPHA_SIZE 261       /* src/main/index_types.h:64-66 */
#define FEMTO_AMD_CHARACTER_OFFSET 5

typedef struct femto_amd_index femto_amd_index_t;   /* opaque; owns the device-resident index */

/* Replaces femto_start_server_err + femto_loc_for_path_err (src/main/femto.c:54,269) and the lazy
 * block faults of open_header_block/open_data_block (src/main/index.c:1482,1419): reads a femto
 * index (directory "<dir>/00","<dir>/01".. per src/main/block_storage.c:257-263, or a flattened
 * single file per src/main/index.c:2260), validates every block header (src/main/index.c:1348),
 * uploads the block images unchanged to HBM of HIP device `device` and builds the small side tables
 * (per-bucket Huffman leaf codes, wavelet-node directory, Occ bases). */
int femto_amd_open(const char* index_path, int device, femto_amd_index_t** out);
void femto_amd_close(femto_amd_index_t* ix);

/* like err_string() of src/utils/error.h:72; thread-local message of the last failing call */
const char* femto_amd_last_error(void);

/* index facts (block header fields, src/main/index.c:817-868) */
typedef struct {
  int64_t total_length;       /* rows of L == prepared text length */
  int64_t number_of_blocks;
  int64_t number_of_documents;
  int32_t block_size, bucket_size, mark_period, chunk_size;
  int32_t text_size_bits;     /* bits per mark-array record */
  int64_t total_buckets;
  int64_t image_bytes;        /* bytes of femto block images resident in HBM */
  int64_t table_bytes;        /* bytes of derived side tables resident in HBM */
} femto_amd_info_t;
int femto_amd_info(const femto_amd_index_t* ix, femto_amd_info_t* out);

/* ---- host-pointer batch API ------------------------------------------------------------- */

/* Replaces parallel_count (src/main/femto.c:275; do_string_query src/main/server.c:713):
 * for pattern i, [first[i], last[i]] is the inclusive row range of the backward search (first>last
 * when there is no match; the empty pattern gives [0, total_length-1]).  If last==NULL, first[i]
 * receives the match count last-first+1 (src/main/femto.c:313-318). */
int femto_amd_parallel_count(femto_amd_index_t* ix, int npats, const int* plen,
                             const uint16_t* const* pats, int64_t* first, int64_t* last);

/* Replaces parallel_locate (src/main/femto.c:331; do_locate_query src/main/server.c:4373):
 * noccs[i] rows are located per pattern, clamped as the reference does (when last-first >
 * max_occs_each only max_occs_each rows are located -- i.e. a range of exactly max_occs_each+1 rows
 * is returned whole, src/main/server.c:4411); offsets[i] is malloc()ed by the callee (NULL when
 * noccs[i]==0) and free()d by the caller; offsets[i][j] = SA[first[i]+j], row order. */
int femto_amd_parallel_locate(femto_amd_index_t* ix, int npats, const int* plen,
                              const uint16_t* const* pats, int max_occs_each,
                              int* noccs, int64_t** offsets);

/* Replaces parallel_locate_range (src/main/femto.c:481; setup_locate_range src/main/server.c:4047): the text offset
 * of every row in [first, last]; offsets must have room for last-first+1 entries.  (serial_locate, femto.c:402, is the
 * reference's single-threaded test twin of parallel_locate: call femto_amd_parallel_locate.) */
int femto_amd_parallel_locate_range(femto_amd_index_t* ix, int64_t first, int64_t last, int64_t* offsets);

/* Flat forms of the two calls above (no per-pattern pointers): pattern i is
 * pats[starts[i] .. starts[i]+plen[i]).  locate_flat writes out_starts[npats+1] (exclusive prefix
 * sum of noccs) and at most offsets_capacity offsets; *total_out receives sum(noccs) -- call with
 * offsets==NULL to size the buffer. */
int femto_amd_count_flat(femto_amd_index_t* ix, int64_t npats, const int32_t* plen,
                         const uint16_t* pats, const int64_t* starts, int64_t* first, int64_t* last);
int femto_amd_locate_flat(femto_amd_index_t* ix, int64_t npats, const int32_t* plen,
                          const uint16_t* pats, const int64_t* starts, int max_occs_each,
                          int32_t* noccs, int64_t* out_starts, int64_t* offsets,
                          int64_t offsets_capacity, int64_t* total_out);

/* One-pass form of locate_flat: *offsets_out receives ONE malloc()ed array holding all offsets (pattern i's are
 * [out_starts[i], out_starts[i+1]); NULL when *total_out == 0); the caller free()s it.  noccs / out_starts may be NULL. */
int femto_amd_locate_flat_alloc(femto_amd_index_t* ix, int64_t npats, const int32_t* plen,
                                const uint16_t* pats, const int64_t* starts, int max_occs_each,
                                int32_t* noccs, int64_t* out_starts, int64_t** offsets_out, int64_t* total_out);

/* Raw-byte convenience form: patterns given as bytes (each +5 -> alpha_t), as femto_search does
 * for literal patterns. */
int femto_amd_count_bytes(femto_amd_index_t* ix, int64_t npats, const int32_t* plen,
                          const uint8_t* bytes, const int64_t* starts, int64_t* first, int64_t* last);

/* Offset -> (document, offset in document): resolve_location (src/main/index.c:1587). */
int femto_amd_resolve_location(const femto_amd_index_t* ix, int64_t offset, int64_t* doc, int64_t* doc_offset);
/* The info string stored with a document (its path/URL): document_info (src/main/index.c:1768).  *info points
 * into memory owned by the handle (valid until femto_amd_close; NOT NUL-terminated), *len its length. */
int femto_amd_document_info(const femto_amd_index_t* ix, int64_t doc, const char** info, int64_t* len);

/* resolve_location for a batch (the reference resolves every located row: one header_loc_query_t each,
 * do_range_to_results_query src/main/server.c:4800-4823): doc[i] / doc_offset[i] for offsets[i]; either output may be NULL.
 * Host arrays; the search runs on the GPU (femto_amd_resolve_device below is the form without the copies). */
int femto_amd_resolve_batch(femto_amd_index_t* ix, int64_t n, const int64_t* offsets, int64_t* doc, int64_t* doc_offset);

/* ---- device-pointer batch API (inputs and outputs already resident in HBM) ---------------- */
/* All pointers are device pointers on the index's device; `stream` is a hipStream_t passed as
 * void* (NULL = default stream).  Calls only enqueue work and return; the caller synchronises.
 * Nothing is reported to the host afterwards: a pattern holding a symbol >= 261 (which the host-pointer
 * calls reject with FEMTO_AMD_ERR_PARAM) has the empty range first = 0, last = -1.
 * READS AROUND THE SYMBOLS: the kernels fetch the patterns in aligned 16-byte pieces, so up to 14 bytes before the first and
 * behind the last symbol of d_pats[] are LOADED (never used, never written).  An aligned piece cannot cross a page, so this
 * cannot fault -- but a memory checker, or a sub-allocator with poisoned guard bytes next to d_pats, will see the reads:
 * give d_pats 16 bytes of slack on either side, or align its ends to 16 bytes, if that matters.  d_pats itself must be
 * 2-byte aligned (FEMTO_AMD_ERR_PARAM otherwise).  (femto_amd_locate_device
 * falls back to a host-synchronising path -- it reads the row total back on `stream` -- for rank modes 0 and 1; the
 * packed modes 3 / 4 are enqueue-only as stated.) */
int femto_amd_count_device(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen,
                           const uint16_t* d_pats, const int64_t* d_starts,
                           int64_t* d_first, int64_t* d_last, void* stream);

/* Locate on device: phase 1 (count + clamp + prefix sum) writes d_noccs[npats] and
 * d_out_starts[npats+1]; the caller reads d_out_starts[npats] (= total) to size d_offsets, then
 * phase 2 walks every row.  d_first must hold the ranges' first rows (phase 1 fills it). */
int femto_amd_locate_plan_device(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen,
                                 const uint16_t* d_pats, const int64_t* d_starts, int max_occs_each,
                                 int64_t* d_first, int64_t* d_last, int32_t* d_noccs,
                                 int64_t* d_out_starts, void* stream);
int femto_amd_locate_walk_device(femto_amd_index_t* ix, int64_t npats, const int64_t* d_first,
                                 const int64_t* d_out_starts, int64_t total, int64_t* d_offsets,
                                 void* stream);

/* The whole of parallel_locate (src/main/femto.c:331) as ONE enqueue-only call: count, the reference's clamp, prefix
 * sum and the locate walk run as one stream-ordered chain; nothing returns to the host in between.  d_offsets has room
 * for offsets_capacity rows; d_total[0] receives the number of rows (= d_out_starts[npats]) and d_total[1] is 1 when
 * that exceeds offsets_capacity (the offsets are then incomplete: call again with a larger buffer).
 * ROW-FREE FORM: d_first == d_last == NULL.  parallel_locate itself returns `noccs` and `offsets` and never a row
 * (src/main/femto.c:331-400); a caller that passes no row arrays gets exactly that -- d_noccs, d_out_starts, d_offsets,
 * d_total, bit-identical to the form with rows -- and the search is spared what only the rows need: on handles holding
 * the text, a pattern whose remaining symbols are compared against the text on ONE row is located by that compare (its
 * offset is where the compared text starts) without the inverse-suffix-array read (and, with sampled arrays, the LF steps)
 * that would turn the position back into a row; a compare that meets another character ends the pattern at once, where the
 * form with rows runs one more step for the (first, last) of the emptied range. */
int femto_amd_locate_device(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen,
                            const uint16_t* d_pats, const int64_t* d_starts, int max_occs_each,
                            int64_t* d_first, int64_t* d_last, int32_t* d_noccs, int64_t* d_out_starts,
                            int64_t* d_offsets, int64_t offsets_capacity, int64_t* d_total, void* stream);
/* femto_amd_locate_device with a STREAMING row plan (femto_amd/plan/plan_stream.hip): same arguments, same contract, every
 * output bit-identical.  On handles that hold the suffix array of every row (rank modes 3 / 4), given an offsets buffer and
 * d_noccs / d_out_starts aligned to 16 bytes, the prefix sum and the row expansion behind the search run as ONE persistent
 * kernel that streams d_noccs in and d_out_starts out -- and nothing runs behind it unless max_occs_each > 4096 lets a range
 * be longer than the cooperative expansion takes.  Every other case (sampled arrays, no offsets buffer, unaligned pointers,
 * rank modes 0 / 1) does what femto_amd_locate_device does.  FEMTO_AMD_PLAN_STREAM=0 switches the streaming kernel off and
 * FEMTO_AMD_PLAN_STREAM_GRID=<workgroups> (tests) fixes its grid; both are read from the environment on every call. */
int femto_amd_locate_device_v2(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen,
                               const uint16_t* d_pats, const int64_t* d_starts, int max_occs_each,
                               int64_t* d_first, int64_t* d_last, int32_t* d_noccs, int64_t* d_out_starts,
                               int64_t* d_offsets, int64_t offsets_capacity, int64_t* d_total, void* stream);
/* Process-wide counters of femto_amd_locate_device_v2 (diagnostics, tests): out[0] calls that took the streaming kernel,
 * out[1] calls that did not, out[2] of out[0] those that launched the long-range kernel behind it, out[3] the workgroups of
 * the last streaming launch. */
void femto_amd_plan_stream_stats(int64_t out[4]);

/* ONE step of the locate walk (do_back_query, src/main/server.c:2228-2359) for n rows, enqueue-only: d_off[i] = the text offset of
 * d_rows[i] when the row is marked (its walk ends here), else -1 and d_next[i] = LF(row) -- -1 when L[row] is a character <= SEOF
 * (a walk does not cross a document start) or the row is out of range.  The unit a RANGE-SPLIT index exchanges walkers in
 * (each round every GPU advances the walkers whose rows it owns -- owner = row / block_size,
 * src/main/index.c:1613-1617 -- and sends each to the owner of its next row): femto_amd/parallel.py exchange_locate.  Marks are the
 * handle's own (the derived, denser ones in modes 3 / 4; femto's in modes 0 / 1): offsets are the same either way. */
int femto_amd_lf_steps_device(femto_amd_index_t* ix, int64_t n, const int64_t* d_rows, int64_t* d_next, int64_t* d_off, void* stream);

/* resolve_location (src/main/index.c:1587) on the device, one lane per offset: d_doc[i] (int64) and / or d_doc32[i] (int32:
 * indexes of fewer than 2^31 documents) = the document holding text offset d_offsets[i], d_doc_offset[i] = the offset inside
 * it; any of the three outputs may be NULL, and d_doc_offset may be d_offsets itself (in place).  d_n != NULL: only
 * min(n, *d_n) offsets are live -- pass the d_total of femto_amd_locate_device and its offsets_capacity as n to resolve the
 * located rows of an enqueue-only chain without a host round trip.  Enqueue-only.  The located offsets of a match are
 * inside a document; an offset at or beyond the last document's end resolves, as in the reference, to document
 * number_of_documents. */
int femto_amd_resolve_device(femto_amd_index_t* ix, const int64_t* d_offsets, int64_t n, const int64_t* d_n, int64_t* d_doc,
                             int32_t* d_doc32, int64_t* d_doc_offset, void* stream);

/* ---- extraction: the text itself (do_context_query, src/main/server.c:2567-2795; do_extract_document_query, :6337-6440) ----
 * T is the prepared text: every document's bytes + 5 followed by SEOF (= 2), total_length positions in all.  Outputs are alpha_t.
 *   EXTRACT BY POSITION: out[out_starts[i] + j] = T[pos[i] + j] for 0 <= j < len[i]; a position outside [0, total_length) is
 *     written as 0.  Ranges may cross documents (the SEOF symbols appear in the output).
 *   EXTRACT A DOCUMENT: T[doc_start, doc_end) -- the document's symbols and its SEOF, doc_len = HDR_LOC_REQUEST_DOC_LEN symbols:
 *     what do_extract_document_query returns (a context query from the document's EOF row, before = doc_len - 1, after = 1).
 *   CONTEXT: anchor p = SA[rows[i]] (rows form) or offsets[i]; before + after slots per anchor, at ctx[i * (before + after)].
 *     Slot before - 1 - j receives T[p - 1 - j] (position -1 wraps to total_length - 1, as L does); the backward walk stops after
 *     it writes the first symbol <= SEOF (do_back_query's rule).  Slot before + j receives T[p + j]; the forward walk stops after
 *     the first symbol <= SEOF (do_forward_query's).  Slots not written are 0 (server.c:2603-2607 zeroes its array likewise; that
 *     array has one spare slot, this one does not).  pos_out[i] (may be NULL) = p (LOCATE_STRONG); a row or offset outside
 *     [0, total_length) gives all zeros and pos_out = -1.
 * The extractor holds what extraction needs beyond the handle.  Handles that hold the text (femto_amd_pack_info bit 4's arrays)
 * copy from it; every other handle -- and FEMTO_AMD_EXTRACT_FORCE_SAMPLES -- uses a table of SA^-1 at every 2^sample_shift-th
 * position (4-byte entries below 2^32 rows; default shift 6: ~67 MB at 1 GiB of text) and the row of every document's SEOF,
 * built on the GPU when the extractor opens, and walks LF back from them: pieces of at most 2^shift positions, one lane each.
 * The table is counted against hbm_budget_bytes: FEMTO_AMD_ERR_MEM (the message says how many bytes) when it does not fit; the
 * handle is unaffected.  Free the extractor before femto_amd_close of its index.  Range-split parts and striped handles:
 * FEMTO_AMD_ERR_INVALID.  Multi-device handle: host forms run on replica 0; device forms FEMTO_AMD_ERR_INVALID. */
typedef struct femto_amd_extractor femto_amd_extractor_t;
#define FEMTO_AMD_EXTRACT_FORCE_SAMPLES 1   /* flags: the sample path even on a handle that holds the text */
#define FEMTO_AMD_EXTRACT_PATH_TEXT 0
#define FEMTO_AMD_EXTRACT_PATH_SAMPLES 1
int femto_amd_extractor_open(femto_amd_index_t* ix, int sample_shift /* -1 auto (6), 0..16 */, int flags, femto_amd_extractor_t** out);
void femto_amd_extractor_free(femto_amd_extractor_t* ex);
/* *path FEMTO_AMD_EXTRACT_PATH_*, *sample_shift (-1 on the text path), *bytes of HBM the extractor holds, *build_ms of its table */
int femto_amd_extractor_info(const femto_amd_extractor_t* ex, int* path, int* sample_shift, int64_t* bytes, double* build_ms);
/* the row of every document's SEOF as the sample table recorded it (the header's doc_eof_rows, index.c:889-897); n = documents */
int femto_amd_extractor_eof_rows(const femto_amd_extractor_t* ex, int64_t* rows, int64_t n);
/* Device forms: enqueue-only on `stream` (the sample path on handles in rank modes 0 / 1 reads its piece count back on `stream`).
 * d_n != NULL (context): only min(n, *d_n) anchors are live, as for femto_amd_resolve_device -- femto_amd_locate_device's
 * d_offsets and d_total chain into a window around every hit without a host round trip; the other anchors' slots are left as
 * they are.  Exactly one of d_rows and d_offsets is non-NULL.  0 <= before, after and before + after <= 2^30. */
int femto_amd_extract_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_pos, const int32_t* d_len,
                             const int64_t* d_out_starts, uint16_t* d_out, void* stream);
int femto_amd_context_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_rows, const int64_t* d_offsets,
                             const int64_t* d_n, int before, int after, uint16_t* d_ctx, int64_t* d_pos_out, void* stream);
/* Host forms (blocking): out_starts NULL = the requests packed one after another; negative lengths or starts: FEMTO_AMD_ERR_PARAM */
int femto_amd_extract(femto_amd_extractor_t* ex, int64_t n, const int64_t* pos, const int32_t* len, const int64_t* out_starts,
                      uint16_t* out);
int femto_amd_context(femto_amd_extractor_t* ex, int64_t n, const int64_t* rows, const int64_t* offsets, int before, int after,
                      uint16_t* ctx, int64_t* pos_out);
/* one whole document: *content (malloc'd, the caller frees it) holds *len = doc_len symbols */
int femto_amd_extract_document(femto_amd_extractor_t* ex, int64_t doc, uint16_t** content, int64_t* len);

/* ---- matching lines: the line around a hit, from the index (print_grep / grep_group_add / complete_grep,
 * src/main_cc/search_tool.cc:134-351, MAX_GREP_LINE = 1024; the file femto_search --grep reads is replaced by the document's bytes
 * as the index holds them) ----
 * THE RULE.  The anchor's document has L = doc_len - 1 bytes b[0 .. L) (byte = symbol - 5; the SEOF is not one of them); o is the
 * anchor's offset in it, 0 <= o <= L.  line_start = line_end = o, then
 *   BACKWARD, i = 1 .. 1023: stop when o - i < 0; stop when b[o - i] is \n or \r; when it is \0 set BINARY and stop; otherwise
 *     line_start = o - i.  The loop running out (1023 bytes, no stop) sets BINARY.
 *   FORWARD, i = 0 .. 1023: stop when o + i >= L; line_end = o + i; stop when b[o + i] is \n or \r; when it is \0 set BINARY and stop.
 *     The loop running out (1024 bytes, no stop) sets BINARY.
 * The line is b[line_start, line_end), line_len = line_end - line_start <= 2046.  As in the reference: a line that runs into the
 * end of the document without a terminator loses its last byte (line_end stays at L - 1); an anchor at o == L (the document's SEOF)
 * gives [line_start, L); an anchor standing on a terminator gives the text before it; BINARY changes neither start nor length (the
 * reference prints "matches" for such a line and groups it like any other).  A line holds no \n, \r or \0.
 * BOUNDS.  Anchors are TEXT offsets -- what femto_amd_locate_device leaves in d_offsets; d_n != NULL: only min(n, *d_n) anchors are
 * live (pass its d_total), the other slots are left as they are.  Outputs, any may be NULL: d_doc[i] the document (numbered as by
 * resolve_location), d_line_pos[i] the TEXT position of the line's start, d_line_len[i], d_flags[i] (FEMTO_AMD_LINE_*).  An anchor
 * outside [0, total_length) gives doc -1, pos -1, len 0 and FEMTO_AMD_LINE_INVALID.
 * BYTES.  The live lines packed one after another as bytes: line i at d_bytes[d_byte_starts[i] .. d_byte_starts[i + 1]);
 * d_byte_starts (n + 1 entries) is the exclusive scan of the lengths (0 for a slot that is not live or has pos < 0).  d_total[0] =
 * the bytes of all lines, d_total[1] = 1 when that exceeds `capacity`: the starts are complete, the bytes are not -- call again
 * with a larger buffer (the protocol of femto_amd_docset_device).
 * GROUPS.  d_group_first[i] = the least j <= i whose line has the same length and the same bytes (grep_group_add's key), -1 for a
 * slot flagged FEMTO_AMD_LINE_INVALID (d_flags may be NULL: none is); *d_ngroups = the number of distinct lines.  Lines are found
 * by a hash and CONFIRMED on their bytes, never by the hash alone.  hash_bits: 0 or 64 the full hash, 1 .. 63 only that many bits of
 * it -- a diagnostic that forces collisions; it changes no output.
 * All three device forms are enqueue-only on `stream` on a handle that holds the text.  Every other extractor (and
 * FEMTO_AMD_EXTRACT_FORCE_SAMPLES) takes the bounds from femto_amd_context_device(1023, 1024) in chunks of 65536 anchors and the
 * bytes from femto_amd_extract_device through at most 256 MiB of scratch, which these calls allocate and free (a device-wide wait).
 * At most 2^31 - 1 anchors per call.  Handles as for extraction: range-split parts and striped handles FEMTO_AMD_ERR_INVALID;
 * multi-device handle: host forms on replica 0, device forms FEMTO_AMD_ERR_INVALID. */
#define FEMTO_AMD_LINE_BINARY 1
#define FEMTO_AMD_LINE_INVALID 2
int femto_amd_lines_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_offsets, const int64_t* d_n, int64_t* d_doc,
                           int64_t* d_line_pos, int32_t* d_line_len, uint8_t* d_flags, void* stream);
int femto_amd_line_bytes_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_n, const int64_t* d_line_pos,
                                const int32_t* d_line_len, int64_t* d_byte_starts /* n + 1 */, uint8_t* d_bytes, int64_t capacity,
                                int64_t* d_total /* 2 */, void* stream);
int femto_amd_line_groups_device(femto_amd_extractor_t* ex, int64_t n, const int64_t* d_n, const int64_t* d_byte_starts,
                                 const uint8_t* d_bytes, const uint8_t* d_flags, int hash_bits, int64_t* d_group_first,
                                 int64_t* d_ngroups, void* stream);
/* Host forms (blocking, host arrays).  femto_amd_lines: bounds and bytes of n anchors; doc, line_pos, line_len, flags may be NULL;
 * byte_starts (n + 1), bytes and total go together (all NULL: bounds only): *bytes is malloc()ed by the callee (NULL when *total =
 * byte_starts[n] is 0) and free()d by the caller, as with femto_amd_locate_flat_alloc.  femto_amd_line_groups: the groups of n
 * packed lines (flags may be NULL). */
int femto_amd_lines(femto_amd_extractor_t* ex, int64_t n, const int64_t* offsets, int64_t* doc, int64_t* line_pos, int32_t* line_len,
                    uint8_t* flags, int64_t* byte_starts /* n + 1 */, uint8_t** bytes, int64_t* total);
int femto_amd_line_groups(femto_amd_extractor_t* ex, int64_t n, const int64_t* byte_starts, const uint8_t* bytes, const uint8_t* flags,
                          int hash_bits, int64_t* group_first, int64_t* ngroups);

/* ---- document listing: which documents match (results_create_sort_locations, src/main/results.c:213; the last step of
 * do_range_to_results_query, src/main/server.c:4549) and AND / OR / NOT of the lists (intersectResults / unionResults /
 * subtractResults, results.c:435 / 497 / 669) ----
 * LISTING.  Input is exactly what femto_amd_locate_device leaves in HBM: d_out_starts[npats + 1], d_offsets[capacity] and
 * d_total[2] (row total, overflow flag).  When the flag is set or the total exceeds `capacity` the rows are incomplete and the
 * call writes NOTHING but *d_status = 1 (else 0; d_status may be NULL) -- as femto_amd_resolve_device and
 * femto_amd_context_device treat d_n.  Outputs use the rows' own ragged layout: pattern i's list is entries
 * [d_out_starts[i], d_out_starts[i] + d_ndocs[i]) of
 *   d_docs (int64) / d_docs32 (int32 twin, indexes of fewer than 2^31 documents): the distinct documents among pattern i's
 *     located rows, ascending;
 *   d_hits (int32): how many of the pattern's located rows lie in each listed document (the reference keeps no such count);
 * entries of a segment beyond d_ndocs[i] are left as they are.  PAIRS FORM (RESULT_TYPE_DOC_OFFSETS): d_pair_doc / d_pair_off
 * [d_out_starts[i] + j] = (document, offset in document) of the segment's rows sorted by document, then by offset -- the order
 * of compare_location_info (results.c:199).  *d_doc_total = the sum of d_ndocs.  Every output may be NULL.
 * Document numbers are resolve_location's: an offset at or beyond the last document's end lists as document
 * number_of_documents, as in femto_amd_resolve_device.  The offsets of one segment lie in [0, 2^b), 2^b the least power of two
 * above total_length (every located offset does).
 * THE LISTS DESCRIBE THE ROWS THAT WERE LOCATED: with a max_occs_each clamp those are the rows parallel_locate returns, not
 * every row of the pattern's range -- a document whose only matches were clamped away is not listed.
 * SIZE CLASSES (femto_amd_doclist_info): a segment of at most wave_max = 64 rows is sorted across the lanes of one wavefront;
 * of at most workgroup_max = 4096 rows in the LDS of one workgroup (32 KB of keys: four workgroups share a CU's 160 KB); a
 * longer one by a segmented radix sort in HBM (rocPRIM; it takes 32-bit row numbers: FEMTO_AMD_ERR_PARAM when capacity >= 2^32
 * -- split the batch).  Segments are binned on the device; the call is enqueue-only.
 * SET OPERATIONS.  A list is a (start, n) view into an array of documents, ascending, no duplicates -- a d_docs above with
 * d_out_starts / d_ndocs, or a result of this call.  Pair k combines d_docs_a[d_a_start[k] .. + d_a_n[k]) with
 * d_docs_b[d_b_start[k] .. + d_b_n[k]) (the two arrays may be the same) by d_op[k]: AND, OR, or NOT = a minus b.  Results are
 * packed: pair k's at [d_res_starts[k], d_res_starts[k + 1]) of d_res_docs; d_res_total[0] = their total, d_res_total[1] = 1
 * when it exceeds res_capacity (d_res_starts is complete, d_res_docs is not: call again with a larger buffer -- the protocol of
 * femto_amd_locate_device).  Hit counts are not carried through.  Enqueue-only.
 * Range-split parts and striped handles: FEMTO_AMD_ERR_INVALID.  Multi-device handle: the host forms run on replica 0, the
 * device forms return FEMTO_AMD_ERR_INVALID.  The listing takes located offsets, so it does not depend on the rank mode. */
#define FEMTO_AMD_DOCSET_AND 0
#define FEMTO_AMD_DOCSET_OR 1
#define FEMTO_AMD_DOCSET_NOT 2
int femto_amd_doclist_info(int* wave_max, int* workgroup_max);
int femto_amd_doclist_device(femto_amd_index_t* ix, int64_t npats, const int64_t* d_out_starts, const int64_t* d_offsets,
                             int64_t capacity, const int64_t* d_total, int32_t* d_ndocs, int64_t* d_docs, int32_t* d_docs32,
                             int32_t* d_hits, int64_t* d_pair_doc, int64_t* d_pair_off, int64_t* d_doc_total, int32_t* d_status,
                             void* stream);
int femto_amd_docset_device(femto_amd_index_t* ix, int64_t npairs, const int64_t* d_docs_a, const int64_t* d_a_start,
                            const int32_t* d_a_n, const int64_t* d_docs_b, const int64_t* d_b_start, const int32_t* d_b_n,
                            const int32_t* d_op, int64_t* d_res_starts /* npairs + 1 */, int64_t* d_res_docs, int64_t res_capacity,
                            int64_t* d_res_total /* 2 */, void* stream);
/* Host forms (blocking, host arrays).  femto_amd_doclist: locate (patterns as in femto_amd_locate_flat, the same clamp) and list;
 * the lists come back PACKED: pattern i's documents and hits are [doc_starts[i], doc_starts[i + 1]) of *docs / *hits, which the
 * callee malloc()s (NULL when *total = doc_starts[npats] is 0) and the caller free()s, as with femto_amd_locate_flat_alloc; hits
 * may be NULL.  femto_amd_docset: the set operations on host lists, results packed into *res_docs (malloc()ed likewise). */
int femto_amd_doclist(femto_amd_index_t* ix, int64_t npats, const int32_t* plen, const uint16_t* pats, const int64_t* starts,
                      int max_occs_each, int64_t* doc_starts /* npats + 1 */, int64_t** docs, int32_t** hits, int64_t* total);
int femto_amd_docset(femto_amd_index_t* ix, int64_t npairs, const int64_t* docs_a, const int64_t* a_start, const int32_t* a_n,
                     const int64_t* docs_b, const int64_t* b_start, const int32_t* b_n, const int32_t* op,
                     int64_t* res_starts /* npairs + 1 */, int64_t** res_docs, int64_t* total);

/* ---- positional operators: THEN / WITHIN / OR of (document, offset in document) lists (thenResults / withinResults,
 * src/main/results.c:732 / 842; unionResults on RESULT_TYPE_DOC_OFFSETS, :497) ----
 * A list is a (start, n) view into a pair of arrays (document, offset in document), strictly ascending in (document, offset) --
 * the PAIRS FORM of femto_amd_doclist_device with d_out_starts and the row counts, for located rows (distinct offsets), or a
 * result of this call.  Job k combines d_a_doc / d_a_off [d_a_start[k] .. + d_a_n[k]) (the LEFT list) with d_b_doc / d_b_off
 * [d_b_start[k] .. + d_b_n[k]) (the RIGHT list; the arrays may be the same) by d_op[k] and the distance d = d_distance[k]:
 *   every left element l meets exactly one right element, the first r >= l, if that lies in l's document; every right element
 *   r meets exactly one left element, the first l > r, if that lies in r's document (the reference's two-pointer loops, which
 *   advance the right side while right < left and the left side otherwise, make exactly these comparisons);
 *   THEN, d > 0: l is in the result iff 0 < r - l <= d ("l, then r within d").  r == l yields nothing, even when a later right
 *     element is in reach -- the reference's behaviour.  THEN, d < 0: r is in the result iff 0 < l - r <= |d|.  d == 0: empty.
 *   WITHIN, any d: l is in the result iff r - l <= |d|, and r iff l - r <= |d|.
 *   OR (d ignored): the union.
 * The result is ascending and holds a position once.  ONE DEPARTURE: when a position stands in both lists and the next left
 * element lies within |d| of it, withinResults appends that position twice and its writer fails with ERR_PARAM
 * (results_writer_append, results.c:294); here it is written once.  An unknown operator yields the empty result.
 * Results are packed: job k's at [d_res_starts[k], d_res_starts[k + 1]) of d_res_doc / d_res_off; d_res_total[0] = their
 * total, d_res_total[1] = 1 when it exceeds res_capacity (d_res_starts is complete, the pair arrays are not: call again with a
 * larger buffer -- the protocol of femto_amd_docset_device).  No result holds more than d_a_n[k] + d_b_n[k] pairs.  Enqueue-only.
 * TILES (femto_amd_docpos_info): the unit of work is `tile` = 2048 positions of one job's merged order, taken by one workgroup
 * that stages the two slices in LDS (32 KB: four workgroups share a CU's 160 KB); the tiles of all jobs are dealt evenly over
 * a persistent grid, so one job of millions of pairs is spread over the whole device.  A job of a few pairs still takes a whole
 * tile -- one workgroup, three barriers: millions of such jobs keep every CU busy but run several times slower per element than
 * long jobs do, and slower than femto_amd_docset_device runs on lists as short (profiles/docpos_stats.txt has the figures).
 * Every call also pays a fixed floor of two scans over 32 768 chunk counts and a walk of the chunks, however few jobs it has.
 * femto_amd_docpos_chunks returns that number of chunks: a call of more tiles than chunks deals several tiles to a chunk.
 * femto_amd_docpos_documents_device: list i = entries [d_starts[i], d_starts[i + 1]) of d_pair_doc (such as d_res_starts /
 * d_res_doc above); its distinct documents, ascending, go to [d_doc_starts[i], d_doc_starts[i + 1]) of d_docs, with d_total[2]
 * and doc_capacity under the same overflow protocol -- a valid operand of femto_amd_docset_device, so AND / OR / NOT apply to
 * THEN / WITHIN results.  Enqueue-only.
 * Handles: as for the document listing (range-split parts and striped handles FEMTO_AMD_ERR_INVALID; multi-device handle: host
 * forms on replica 0, device forms FEMTO_AMD_ERR_INVALID). */
#define FEMTO_AMD_DOCPOS_THEN 0
#define FEMTO_AMD_DOCPOS_WITHIN 1
#define FEMTO_AMD_DOCPOS_OR 2
int femto_amd_docpos_info(int* tile);
int femto_amd_docpos_chunks(void);
int femto_amd_docpos_device(femto_amd_index_t* ix, int64_t npairs, const int64_t* d_a_doc, const int64_t* d_a_off,
                            const int64_t* d_a_start, const int32_t* d_a_n, const int64_t* d_b_doc, const int64_t* d_b_off,
                            const int64_t* d_b_start, const int32_t* d_b_n, const int32_t* d_op, const int32_t* d_distance,
                            int64_t* d_res_starts /* npairs + 1 */, int64_t* d_res_doc, int64_t* d_res_off, int64_t res_capacity,
                            int64_t* d_res_total /* 2 */, void* stream);
int femto_amd_docpos_documents_device(femto_amd_index_t* ix, int64_t nlists, const int64_t* d_starts /* nlists + 1 */,
                                      const int64_t* d_pair_doc, int64_t* d_doc_starts /* nlists + 1 */, int64_t* d_docs,
                                      int64_t doc_capacity, int64_t* d_total /* 2 */, void* stream);
/* Host forms (blocking, host arrays; parameter errors -- negative counts or starts, an unknown operator, NULL where a pointer is
 * required -- are FEMTO_AMD_ERR_PARAM before any device work).  femto_amd_docpos: the operators on host lists; the results come
 * back packed in *res_doc / *res_off, which the callee malloc()s (NULL when *total = res_starts[npairs] is 0) and the caller
 * free()s.  femto_amd_proximity: the whole job for npairs pattern pairs (each side flat, as in femto_amd_locate_flat): locate
 * both sides, list them in pairs form, combine, copy back once; between the steps only the row total is read back, to size the
 * buffers.  THE LISTS DESCRIBE THE ROWS THAT WERE LOCATED: with a max_occs_each clamp a result is the operator applied to the
 * rows parallel_locate returns for either pattern, not to every occurrence. */
int femto_amd_docpos(femto_amd_index_t* ix, int64_t npairs, const int64_t* a_doc, const int64_t* a_off, const int64_t* a_start,
                     const int32_t* a_n, const int64_t* b_doc, const int64_t* b_off, const int64_t* b_start, const int32_t* b_n,
                     const int32_t* op, const int32_t* distance, int64_t* res_starts /* npairs + 1 */, int64_t** res_doc,
                     int64_t** res_off, int64_t* total);
int femto_amd_proximity(femto_amd_index_t* ix, int64_t npairs, const int32_t* l_plen, const uint16_t* l_pats, const int64_t* l_starts,
                        const int32_t* r_plen, const uint16_t* r_pats, const int64_t* r_starts, const int32_t* op,
                        const int32_t* distance, int max_occs_each, int64_t* res_starts /* npairs + 1 */, int64_t** res_doc,
                        int64_t** res_off, int64_t* total);

/* ---- common sequences (src/main/similar_tool.c): which byte sequences a file that is probably NOT in the index shares with it,
 * which documents share them, and how similar the file is to each ----
 * TAKEN FROM THE REFERENCE: the definitions of its header comment (similar_tool.c:49-84), its score (accumulate_score /
 * compute_score, :207-253) and its defaults min_match_length = 8 and max_offsets = 100.  femto-similar itself is not rebuilt and its
 * printout is not restated: the --too-similar-stop early exit, "a sequence is reported only when none of its occurrences extends"
 * and the overlap removal in qsort order are heuristics of that tool.
 * MATCHING STATISTICS.  For every END position j of the query bytes q[0 .. n): d_len[j] = the largest l in [0, min(j + 1, max_len)]
 * such that q[j - l + 1 .. j], as alpha codes byte + 5, occurs in the index, and (d_first[j], d_last[j]) = the inclusive range
 * parallel_count returns for that string -- for l = 0 the empty pattern's range (0, total_length - 1): the range at j is always what
 * femto_amd_count_device answers for the reported substring.  d_first and d_last may both be NULL.  max_len <= 0: 32768
 * (MAX_PATTERN_LENGTH).  n = 0: nothing is done.  A match never crosses a document boundary (bytes never map to a code <= SEOF).
 * One lane per end position runs the backward search until its range empties; nothing returns to the host.
 * READS AROUND THE BYTES: d_bytes is fetched in aligned 8-byte words, so up to 7 bytes before d_bytes[0] and behind d_bytes[n - 1]
 * are LOADED (never used, never written).  An aligned word cannot cross a page, so this cannot fault; give d_bytes 8 bytes of slack
 * on either side, or align its ends to 8 bytes, if a memory checker matters (as with d_pats of femto_amd_count_device).
 * Rank modes 3 / 4: every layout.  Rank modes 0 / 1: handles with the derived segment lines (the rule of
 * femto_amd_nfa_search_batch), FEMTO_AMD_ERR_INVALID otherwise.  femto_amd_match_stats_steps_device is the same search with no
 * outputs but two counters (diagnostics, tools/similar_bench.py): d_steps[0] = search steps taken, d_steps[1] = those that started
 * from a range of ONE row.
 * SEQUENCES.  End position j is selected when d_len[j] >= min_len and (j == n - 1 or d_len[j + 1] <= d_len[j]): the match ending at
 * j is not contained in the one ending at j + 1 (d_len[j + 1] <= d_len[j] + 1 always holds).  min_len <= 0: 8.  The selected
 * sequences are written in ascending j: start = j - len + 1, len, first, last (each output may be NULL); d_total[0] = their number,
 * d_total[1] = 1 when it exceeds `capacity` (the protocol of femto_amd_locate_device).
 * GROUPS.  The distinct strings among the min(d_total[0], capacity) sequences.  Two sequences are the same string exactly when
 * (len, first) are equal -- the ranges of distinct strings of one length are disjoint -- so grouping is one sort of the 64-bit keys
 * (65535 - len) << 48 | first and no byte is compared: lengths above 65535 are not told apart.  Groups are ordered by length
 * descending, then first ascending; d_g_here = the group's number of selected sequences, d_g_min_start = its smallest start,
 * d_group_of[k] = the group of sequence k (each output but d_ngroups may be NULL; the group arrays need room for `capacity`
 * groups).  d_ngroups[0] = the groups, d_ngroups[1] = the index score's numerator: the sum over groups of
 * len * min(here, last - first + 1).
 * DOCUMENTS.  For every group g < min(d_ngroups[0], ngroups_capacity) with d_g_keep[g] != 0 (NULL: all): its rows under
 * do_locate_query's clamp (the first max_occs_each rows when the range holds more than max_occs_each + 1; <= 0: 100) are located
 * (femto_amd_locate_walk_device) and listed (femto_amd_doclist_device: h(g, d) = located rows in document d); then
 * d_doc_score[d] += len_g * min(here_g, h(g, d)) and d_doc_seqs[d] += 1.  Both accumulators are dense, number_of_documents
 * entries, zeroed by the call.  d_offsets (offsets_capacity entries) receives the located offsets; d_total[0] = the rows,
 * d_total[1] = 1 when they exceed offsets_capacity: nothing is accumulated then -- call again with a larger buffer.  The walk is
 * sized on the host, min(offsets_capacity, ngroups_capacity * max_occs_each) rows: size both capacities to what is expected.
 * THE SCORES DESCRIBE THE ROWS THAT WERE LOCATED, as the document lists do.
 * All device forms are enqueue-only; temporaries come from the handle's scratch.  Range-split parts and striped handles:
 * FEMTO_AMD_ERR_INVALID.  Multi-device handle: the host form runs on replica 0, the device forms return FEMTO_AMD_ERR_INVALID. */
int femto_amd_match_stats_device(femto_amd_index_t* ix, int64_t n, const uint8_t* d_bytes, int32_t max_len, int32_t* d_len,
                                 int64_t* d_first, int64_t* d_last, void* stream);
int femto_amd_match_stats_steps_device(femto_amd_index_t* ix, int64_t n, const uint8_t* d_bytes, int32_t max_len,
                                       int64_t* d_steps /* 2 */, void* stream);
int femto_amd_common_sequences_device(femto_amd_index_t* ix, int64_t n, const int32_t* d_len, const int64_t* d_first,
                                      const int64_t* d_last, int32_t min_len, int64_t* d_seq_start, int32_t* d_seq_len,
                                      int64_t* d_seq_first, int64_t* d_seq_last, int64_t capacity, int64_t* d_total /* 2 */,
                                      void* stream);
int femto_amd_common_groups_device(femto_amd_index_t* ix, int64_t capacity, const int64_t* d_total, const int64_t* d_seq_start,
                                   const int32_t* d_seq_len, const int64_t* d_seq_first, const int64_t* d_seq_last,
                                   int64_t* d_group_of, int32_t* d_g_len, int64_t* d_g_first, int64_t* d_g_last, int32_t* d_g_here,
                                   int64_t* d_g_min_start, int64_t* d_ngroups /* 2: groups, sum of len * min(here, there) */,
                                   void* stream);
int femto_amd_similar_documents_device(femto_amd_index_t* ix, int64_t ngroups_capacity, const int64_t* d_ngroups,
                                       const int32_t* d_g_len, const int64_t* d_g_first, const int64_t* d_g_last,
                                       const int32_t* d_g_here, const uint8_t* d_g_keep, int max_occs_each, int64_t* d_offsets,
                                       int64_t offsets_capacity, int64_t* d_doc_score, int32_t* d_doc_seqs, int64_t* d_total /* 2 */,
                                       void* stream);
/* Host form (blocking): uploads the bytes and runs the chain above.  n_not > 0: the groups' bytes (q[min_start .. min_start + len)
 * + 5) are counted with femto_amd_count_device on every stop-list handle not_ix[k] -- each on the device of `ix`, FEMTO_AMD_ERR_INVALID
 * otherwise -- and a group that occurs in any of them is dropped (kept = 0): it adds to no score.  max_len > 65535:
 * FEMTO_AMD_ERR_PARAM.  n = 0: an empty result.  Every array of the result is malloc()ed by the callee (NULL when empty) and released
 * by femto_amd_similar_free: len[n]; the groups' g_len, g_first, g_last, g_here, g_min_start, g_kept [ngroups], in the order of
 * femto_amd_common_groups_device; index_numerator = the kept groups' sum of len * min(here, last - first + 1) and index_score =
 * index_numerator / n; the ndocs documents with a non-zero score: doc, doc_numerator, doc_seqs and doc_score = doc_numerator /
 * min(n, the document's bytes) (compute_score's divisor), by score descending, then document ascending. */
typedef struct femto_amd_similar_result {
  int64_t n;
  int32_t* len;
  int64_t ngroups;
  int32_t* g_len;
  int64_t* g_first;
  int64_t* g_last;
  int32_t* g_here;
  int64_t* g_min_start;
  uint8_t* g_kept;
  int64_t index_numerator;
  double index_score;
  int64_t ndocs;
  int64_t* doc;
  int64_t* doc_numerator;
  int32_t* doc_seqs;
  double* doc_score;
} femto_amd_similar_result_t;
int femto_amd_similar(femto_amd_index_t* ix, const uint8_t* bytes, int64_t n, int32_t min_len, int32_t max_len, int max_occs_each,
                      int n_not, femto_amd_index_t* const* not_ix, femto_amd_similar_result_t* out);
void femto_amd_similar_free(femto_amd_similar_result_t* out);

/* ---- search with substitutions (k-mismatch): where does a string occur with at most k characters changed?  The substitution-only
 * case of APPROX max:subst:delete:insert (src/main/QUERY_FORMAT.txt:129-160, do_regexp_query) for batches of plain strings ----
 * TAKEN FROM THE REFERENCE: the question, its bound of two edits (QUERY_FORMAT.txt:138, compile_regexp.c:683-685) and the order of
 * its result list (regexp_result_list_sort, src/main/server.c:1528).  NOT TAKEN: the automaton, and with it the rule that the LAST
 * character of the pattern is never substituted (QUERY_FORMAT.txt:143): HERE THE LAST CHARACTER IS SUBSTITUTED LIKE ANY OTHER, so
 * this call finds variants that femto_amd_regexp_search_approx does not.  Insertions and deletions: femto_amd_edit, below.
 * THE QUESTION.  A pattern is a string of alpha codes (byte + 5).  Its substitutable positions are those holding a byte character
 * (code >= FEMTO_AMD_CHARACTER_OFFSET); the substitutes are the byte characters that occur in the text (C[ch + 1] > C[ch]) other than
 * the pattern's own character at that position.  A variant of cost c is the pattern with c substitutions at c different positions.
 * The answer for pattern q and bound k (0, 1 or 2; anything else: FEMTO_AMD_ERR_PARAM) is every variant of cost <= k whose row range
 * is not empty, with (first, last) = what femto_amd_count_device returns for the variant as a pattern of its own, its cost, and its
 * substitutions: d_sub_pos[2 r], d_sub_pos[2 r + 1] = their positions from the left in ascending order, -1 for an unused slot, and
 * d_sub_sym[2 r], [2 r + 1] = the substitutes' alpha codes (0 for an unused slot).  Results stand in batch order of their patterns
 * and, within a pattern, by first ascending: the variants of one pattern have one length, so their ranges are disjoint and first is
 * a unique key.  Pattern q's results are entries d_result_start[q] .. d_result_start[q + 1] - 1.
 * k = 0 is femto_amd_count_device: one result of cost 0 where the pattern occurs, none otherwise.  A pattern character that the text
 * lacks (an N in a DNA read) empties every exact step through it, and is substituted like any other.  A position holding a code
 * below FEMTO_AMD_CHARACTER_OFFSET (SEOF and its neighbours) is matched exactly and never substituted, and no substitute is such a
 * code.  The empty pattern has the one result (0, total_length - 1) of cost 0.  A pattern holds at most 32768 symbols: the host
 * form answers FEMTO_AMD_ERR_PARAM, the device form -- which never reads d_starts on the host -- gives such a pattern no results.
 * DEVICE FORM.  Enqueue-only on the caller's stream: no host synchronisation, no copy to the host; temporaries come from the
 * handle's scratch.  Pattern q = d_syms[d_starts[q] .. d_starts[q + 1]); nsyms = d_starts[npat], by value (npat = 0 needs nsyms = 0:
 * d_result_start[0] = 0 and d_total = {0, 0}).  d_total[0] = the results in all, d_total[1] = 1 when they exceed `capacity`;
 * d_result_start and d_total[0] are exact whatever the capacity.  capacity = 0: the five result arrays may be NULL -- the counting
 * form.  On overflow only d_result_start and d_total are defined: call again with capacity = d_total[0].  npat, nsyms and capacity
 * are below 2^31, FEMTO_AMD_ERR_PARAM otherwise; nothing else bounds a batch: the lanes of the substitution pass (nsyms times the
 * byte characters of the text, up to 2^39) go out in as many launches as they need.  Rank modes 3 / 4: every layout.  Rank modes 0 / 1: handles with the derived segment lines,
 * FEMTO_AMD_ERR_INVALID otherwise.  Range-split parts and striped handles: FEMTO_AMD_ERR_INVALID.  Multi-device handle: the host
 * form runs on replica 0, the device form returns FEMTO_AMD_ERR_INVALID.  The level table and the hash tables are not used.
 * WHAT THE DEVICE FORM IS HANDED.  d_starts and d_syms are read on the device alone, so nothing in them is refused; the kernels
 * bound what a bad entry can do.  A pattern whose bounds leave [0, nsyms] (d_starts[q] < 0 or d_starts[q + 1] > nsyms) or whose
 * length d_starts[q + 1] - d_starts[q] is negative has no results, as a pattern of more than 32768 symbols has none; nothing of it
 * is read, and the patterns beside it have the results they have alone.  Symbols of d_syms that no pattern covers -- in front of
 * d_starts[0], behind d_starts[npat], inside a pattern without results -- are ignored.  A symbol >= FEMTO_AMD_ALPHA_SIZE, which the
 * host form refuses, matches nothing and is never substituted: its pattern has no results.  Patterns that OVERLAP in d_syms
 * (descending starts that leave two well-formed patterns sharing symbols) are not supported: their results are not defined. */
int femto_amd_mismatch_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms,
                              const int64_t* d_starts /* npat + 1 */, int k, int64_t capacity, int64_t* d_result_start /* npat + 1 */,
                              int64_t* d_first, int64_t* d_last, int32_t* d_cost, int32_t* d_sub_pos /* 2 per result */,
                              uint16_t* d_sub_sym /* 2 per result */, int64_t* d_total /* 2 */, void* stream);
/* Host form (blocking): pattern i = the plen[i] symbols of `syms` that follow those of pattern i - 1 (pageable host arrays).  A
 * counting pass (capacity 0) sizes the filling pass.  Every array of the result is malloc()ed by the callee and released by
 * femto_amd_mismatch_free: result_start[npat + 1]; first, last, cost [total]; sub_pos, sub_sym [2 * total] (NULL when total = 0).
 * A symbol >= FEMTO_AMD_ALPHA_SIZE, a pattern of more than 32768 symbols: FEMTO_AMD_ERR_PARAM.  2^31 results or more:
 * FEMTO_AMD_ERR_FULL. */
typedef struct femto_amd_mismatch_result {
  int64_t npat;
  int64_t total;
  int64_t* result_start;
  int64_t* first;
  int64_t* last;
  int32_t* cost;
  int32_t* sub_pos;
  uint16_t* sub_sym;
} femto_amd_mismatch_result_t;
int femto_amd_mismatch(femto_amd_index_t* ix, int64_t npat, const int32_t* plen, const uint16_t* syms, int k,
                       femto_amd_mismatch_result_t* out);
void femto_amd_mismatch_free(femto_amd_mismatch_result_t* out);

/* ---- search within edit distance: which strings that occur in the text are at most k substitutions, deletions and insertions away
 * from a pattern?  APPROX k:1:1:1 (src/main/QUERY_FORMAT.txt:129-160, do_regexp_query) for batches of plain strings ----
 * TAKEN FROM THE REFERENCE: the question, its unit costs and its bound of two edits (QUERY_FORMAT.txt:138, compile_regexp.c:683-685).
 * NOT TAKEN: the automaton and what follows from how it is searched.  THE REFERENCE (1) NEVER EXTENDS A MATCH THAT HAS REACHED A FINAL
 * STATE, (2) DROPS RANGES THAT LIE INSIDE ANOTHER (regexp_result_list_sort, src/main/server.c:1528-1573) AND (3) NEVER SUBSTITUTES THE
 * LAST CHARACTER (QUERY_FORMAT.txt:143); THIS CALL LISTS EVERY STRING.  It therefore contains what femto_amd_regexp_search_approx finds
 * for k:1:1:1 -- under the same (first, length) and last, at a cost no higher -- and more.
 * THE QUESTION.  A pattern is a string of m alpha codes, as for femto_amd_mismatch; the bound is k = 0, 1 or 2 (anything else:
 * FEMTO_AMD_ERR_PARAM).  Three operations, each of cost 1: SUBSTITUTE a byte code of the pattern (a code in [5, 261)) by another byte
 * character that occurs in the text (C[ch + 1] > C[ch]); DELETE a byte code of the pattern; INSERT a byte character that occurs in the
 * text into any of the m + 1 gaps, both ends included -- but for a gap whose left neighbour in the pattern is a code below
 * FEMTO_AMD_CHARACTER_OFFSET: that would put SEOF inside the variant, where femto_amd_count_device does not see text joined across
 * documents.  Codes below FEMTO_AMD_CHARACTER_OFFSET are matched exactly: never substituted, deleted or inserted.
 * The answer for pattern q is every DISTINCT string v that at most k operations reach and whose row range is not empty, with
 *   d_first, d_last = what femto_amd_count_device returns for v as a pattern of its own,
 *   d_length        = the symbols of v, between m - k and m + k,
 *   d_cost          = the FEWEST operations that reach v (for a pattern of bytes alone: the Levenshtein distance).  A string reached
 *                     at cost 1 and at cost 2 is ONE result of cost 1; the pattern itself, reached by an insertion and a deletion, is
 *                     one result of cost 0.
 * The empty string is a result when m <= k and every symbol is a byte code: (0, total_length - 1), length 0.
 * NO EDIT SCRIPT IS RETURNED: a minimal script is not unique, and the caller has the pattern and -- through femto_amd_extract* -- the
 * string.
 * ORDER.  Patterns stand in batch order; pattern q's results are entries d_result_start[q] .. d_result_start[q + 1] - 1, sorted by
 * first ascending, then length ascending.  (first, length) is a unique key -- two strings of one length with the same first row are
 * the same string -- and this is the lexicographic order of the codes with a prefix in front of its extensions.  THE RANGES OF ONE
 * PATTERN MAY NEST, unlike those of femto_amd_mismatch: "ab" holds "abc".  A caller who wants every text position once drops the
 * ranges that lie inside another, as regexp_result_list_sort does (src/main/server.c:1528-1573).
 * CAPACITY.  Several scripts reach one string, so the distinct results cannot be counted without storing records: `capacity` bounds the
 * RAW records the search emits, from which the results are de-duplicated.  d_total[2] = the raw records emitted, exact whatever the
 * capacity; d_total[1] = 1 when they exceed `capacity`; d_total[0] = the distinct results, defined only without overflow.
 * capacity = 0 is the counting form: d_result_start and the four result arrays may be NULL and only d_total[1] and d_total[2] are
 * defined.  On overflow likewise: call again with capacity = d_total[2].  Without overflow d_result_start[npat + 1] and the first
 * d_total[0] entries of the four arrays hold the results (the arrays need `capacity` entries each).
 * DEVICE FORM.  Enqueue-only on the caller's stream: no host synchronisation, no copy to the host, no allocation once the handle's
 * scratch has grown to the batch; it can be captured into a graph like its siblings.  Pattern q = d_syms[d_starts[q] .. d_starts[q + 1]);
 * nsyms = d_starts[npat], by value (npat = 0 needs nsyms = 0: d_result_start[0] = 0 and d_total = {0, 0, 0}).  npat, nsyms and capacity
 * are below 2^31, FEMTO_AMD_ERR_PARAM otherwise; a pattern holds at most 32768 symbols.  The lanes of the edit pass -- (nsyms + npat)
 * sites times twice the byte characters of the text plus one -- go out in as many launches as they need.  Rank modes 3 / 4: every
 * layout.  Rank modes 0 / 1: handles with the derived segment lines, FEMTO_AMD_ERR_INVALID otherwise.  Range-split parts and striped
 * handles: FEMTO_AMD_ERR_INVALID.  Multi-device handle: the host form runs on replica 0, the device form returns
 * FEMTO_AMD_ERR_INVALID.  The level table and the hash tables are not used.
 * WHAT THE DEVICE FORM IS HANDED is bounded exactly as for femto_amd_mismatch_device: a pattern whose bounds leave [0, nsyms], whose
 * length is negative or above 32768 has no results and nothing of it is read; symbols that no pattern covers are ignored; a symbol
 * >= FEMTO_AMD_ALPHA_SIZE matches nothing and is never substituted or deleted: its pattern has no results.  The patterns beside such a
 * pattern have the results they have alone.  Patterns that overlap in d_syms are not supported. */
int femto_amd_edit_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms,
                          const int64_t* d_starts /* npat + 1 */, int k, int64_t capacity, int64_t* d_result_start /* npat + 1 */,
                          int64_t* d_first, int64_t* d_last, int32_t* d_cost, int32_t* d_length, int64_t* d_total /* 3 */, void* stream);
/* Host form (blocking): pattern i = the plen[i] symbols of `syms` that follow those of pattern i - 1 (pageable host arrays).  A
 * counting pass (capacity 0) sizes the filling pass by the raw records.  Every array of the result is malloc()ed by the callee and
 * released by femto_amd_edit_free: result_start[npat + 1]; first, last, cost, length [total] (NULL when total = 0).  A symbol
 * >= FEMTO_AMD_ALPHA_SIZE, a pattern of more than 32768 symbols: FEMTO_AMD_ERR_PARAM.  2^31 raw records or more: FEMTO_AMD_ERR_FULL. */
typedef struct femto_amd_edit_result {
  int64_t npat;
  int64_t total;
  int64_t* result_start;
  int64_t* first;
  int64_t* last;
  int32_t* cost;
  int32_t* length;
} femto_amd_edit_result_t;
int femto_amd_edit(femto_amd_index_t* ix, int64_t npat, const int32_t* plen, const uint16_t* syms, int k,
                   femto_amd_edit_result_t* out);
void femto_amd_edit_free(femto_amd_edit_result_t* out);

/* ---- search with character classes: where do the strings occur that a pattern of fixed length allows, when some of its positions
 * allow a SET of characters?  Case-insensitive search (icase_ast, src/main/ast.c:556, turns every letter into a two-member set),
 * IUPAC codes and N in DNA reads, `[0-9]`, `[^a-z ]` and `.` of the query language -- for batches of patterns, without an automaton ----
 * TAKEN FROM THE REFERENCE: what a set, a period and --icase mean (set_node_invert ast.c:324 and period_range ast.c:33 complement and
 * fill WITHIN THE 256 BYTES) and the order of its result list (regexp_result_list_sort, src/main/server.c:1528).  NOT TAKEN: the
 * automaton: the search is the backward search of femto_amd_count_device with every member of the class tried at a class position.
 * THE QUESTION.  A pattern is a string of uint16 symbols.  A symbol below FEMTO_AMD_ALPHA_SIZE is a literal alpha code, matched
 * exactly -- SEOF and its neighbours included, as in femto_amd_mismatch.  A symbol FEMTO_AMD_CLASS_SYMBOL | c, c < nclasses, names
 * class c of the table the caller passes: d_classes is uint64[4 * nclasses], and bit b of word w of a class says that byte 64 w + b
 * belongs to it.  Classes hold bytes only.  nclasses <= FEMTO_AMD_MAX_CLASSES.
 * The answer for pattern q of m symbols is every DISTINCT string v of m alpha codes such that v[i] equals the literal at every literal
 * position, v[i] - FEMTO_AMD_CHARACTER_OFFSET is in the class at every class position, and the row range of v is not empty; with
 * (first, last) = what femto_amd_count_device returns for v as a pattern of its own.  Results stand in batch order of their patterns
 * and, within a pattern, by first ascending: the strings of one pattern have one length, so their ranges are disjoint and first is a
 * unique key (it is the lexicographic order of their codes).  Pattern q's results are entries d_result_start[q] ..
 * d_result_start[q + 1] - 1.  The empty pattern has the one result (0, total_length - 1).  A class with no member that occurs in the
 * text gives its pattern no results.
 * THE AUTOMATON ROUTE CAN LIST LESS for the same pattern written in the query language: do_regexp_query keeps its pending entries by
 * row range and never extends an entry with a final state alive, so a string that matches the pattern's last k symbols and a shorter
 * one that matches its last j are merged when their ranges are equal (every occurrence of the shorter is followed by the rest of the
 * longer), and strings behind the merged entry are never reached.  This call lists every string; femto_amd_regexp_search's list is a
 * sub-list of it, and the same list where the text has no such pair.
 * NO STRING IS RETURNED, as with femto_amd_edit: the caller has the pattern, and femto_amd_extract* give the text at a row.
 * DEVICE FORM.  Enqueue-only on the caller's stream: no host synchronisation, no copy to the host; temporaries come from the handle's
 * scratch.  Pattern q = d_syms[d_starts[q] .. d_starts[q + 1]); nsyms = d_starts[npat], by value (npat = 0 needs nsyms = 0:
 * d_result_start[0] = 0 and d_total = {0, 0}).  d_total[0] = the results in all, d_total[1] = 1 when they exceed `capacity`.  Every
 * string is reached exactly once, so d_result_start and d_total[0] are exact whatever the capacity.  capacity = 0: d_first and d_last
 * may be NULL -- the counting form.  On overflow only d_result_start and d_total are defined: call again with capacity = d_total[0].
 * npat, nsyms and capacity are below 2^31, FEMTO_AMD_ERR_PARAM otherwise, as are nclasses outside 0 .. 4096 and a NULL d_classes with
 * nclasses > 0.  Handles are served and refused exactly as by femto_amd_mismatch_device: rank modes 3 / 4 every layout; rank modes
 * 0 / 1 handles with the derived segment lines, FEMTO_AMD_ERR_INVALID otherwise; range-split parts and striped handles
 * FEMTO_AMD_ERR_INVALID; multi-device handle: the host form runs on replica 0, the device form returns FEMTO_AMD_ERR_INVALID.
 * WHAT THE DEVICE FORM IS HANDED.  d_starts, d_syms and d_classes are read on the device alone.  A pattern has no results -- and the
 * patterns beside it have the results they have alone -- if its bounds leave [0, nsyms], if its length is negative or above 32768
 * (nothing of such a pattern is read), or if it holds a symbol that is neither a literal below FEMTO_AMD_ALPHA_SIZE nor a class below
 * nclasses.  Patterns that OVERLAP in d_syms are not supported, as for femto_amd_mismatch_device: the search keeps its stack per
 * symbol of d_syms.
 * KNOWN LIMIT.  One GPU lane searches one pattern, depth first.  The number of class positions is bounded by the pattern's length
 * alone, but a pattern with an enormous fan-out -- "...." over a byte text -- is searched serially by its lane: a batch is as slow
 * as its widest pattern. */
#define FEMTO_AMD_CLASS_SYMBOL 0x8000
#define FEMTO_AMD_MAX_CLASSES 4096
int femto_amd_classes_device(femto_amd_index_t* ix, int64_t npat, int64_t nsyms, const uint16_t* d_syms,
                             const int64_t* d_starts /* npat + 1 */, int64_t nclasses, const uint64_t* d_classes /* 4 per class */,
                             int64_t capacity, int64_t* d_result_start /* npat + 1 */, int64_t* d_first, int64_t* d_last,
                             int64_t* d_total /* 2 */, void* stream);
/* Host form (blocking): pattern i = the plen[i] symbols of `syms` that follow those of pattern i - 1 (pageable host arrays).  A
 * counting pass (capacity 0) sizes the filling pass.  Every array of the result is malloc()ed by the callee and released by
 * femto_amd_classes_free: result_start[npat + 1]; first, last [total] (NULL when total = 0).  A symbol that is neither a literal nor
 * a class below nclasses, a pattern of more than 32768 symbols: FEMTO_AMD_ERR_PARAM.  2^31 results or more: FEMTO_AMD_ERR_FULL. */
typedef struct femto_amd_classes_result {
  int64_t npat;
  int64_t total;
  int64_t* result_start;
  int64_t* first;
  int64_t* last;
} femto_amd_classes_result_t;
int femto_amd_classes(femto_amd_index_t* ix, int64_t npat, const int32_t* plen, const uint16_t* syms, int64_t nclasses,
                      const uint64_t* classes, femto_amd_classes_result_t* out);
void femto_amd_classes_free(femto_amd_classes_result_t* out);
/* One query text of the query language (femto_amd_regexp_compile, below, names it) -> its class pattern.  Host only; no handle.
 * The text is parsed by the same parser; with FEMTO_AMD_QUERY_ICASE in `flags`, icase_ast widens it.  A character or a string gives
 * literals, a set or a period a class; a set with ONE member becomes a literal; equal sets share a class number.  *nsyms and
 * *nclasses = what the query needs; when either exceeds its capacity (syms_cap symbols, classes_cap classes of four words) nothing
 * is written and the call returns FEMTO_AMD_ERR_FULL.  FEMTO_AMD_ERR_INVALID when the query is not a concatenation of characters,
 * strings, sets and periods: a repeat operator (also one that streamline_query would trim away: "a+b"), an alternative, a group,
 * APPROX, a boolean operator, a set that holds a code below the bytes beside other members.  A syntax error: FEMTO_AMD_ERR_PARAM. */
int femto_amd_class_pattern_compile(const uint8_t* query, int64_t len, int flags /* FEMTO_AMD_QUERY_ICASE */, uint16_t* syms,
                                    int64_t syms_cap, int64_t* nsyms, uint64_t* classes, int64_t classes_cap, int64_t* nclasses);

/* ---- occurrences within k substitutions, by exact seeds: at which text offsets does a string occur with at most k characters
 * changed?  The question of femto_amd_mismatch for any k up to 255, answered as OFFSETS with a cost rather than as strings with row
 * ranges, and without enumerating a string: the pattern is cut into k + 1 pieces, the pieces are located exactly, and the windows
 * they point at are compared against the text (femto_amd/hamming/hamming.hip; DESIGN.md "Occurrences within k substitutions") ----
 * THE QUESTION.  T is the prepared text of "extraction" above (not cyclic).  A pattern is m alpha codes, BYTE CHARACTERS ONLY
 * (FEMTO_AMD_CHARACTER_OFFSET <= code < FEMTO_AMD_ALPHA_SIZE).  A window p, 0 <= p <= total_length - m, is an occurrence of cost c
 * when T[p + j] != pattern[j] at exactly c <= k positions j and T[p + j] is itself a byte character at each of them: SEOF and its
 * neighbours are never substitutes (the rule of femto_amd_mismatch), so a window never runs over a document's end.  A pattern
 * character that the text lacks (an N in a DNA read) costs one wherever it stands.  The answer for pattern q is every occurrence as
 * (offset p, cost), offsets ascending; patterns stand in batch order; pattern q's results are entries d_result_start[q] ..
 * d_result_start[q + 1] - 1.  For k <= 2 these are exactly the located rows of femto_amd_mismatch's variants, with the variants'
 * costs.  Anchoring at a document's end (a pattern that ends in SEOF) is not offered.
 * BOUNDS.  0 <= k <= 255; k < m <= 32768 (a piece is never empty: the empty string matches every row).
 * PIECES.  Piece j of a pattern covers its positions [j m / (k + 1), (j + 1) m / (k + 1)) in integer division, j = 0 .. k.  This is
 * part of the contract because the CANDIDATES are counted: d_total[2] = the sum, over all pieces of all served patterns, of
 * last - first + 1 as femto_amd_count_device returns it for the piece.  d_total[3] = 1 when that sum exceeds cand_capacity: then only
 * d_total[2] and d_total[3] are defined -- call again with cand_capacity = d_total[2].  An occurrence that holds several pieces
 * unchanged is reported once (by its leftmost such piece).
 * DEVICE FORM.  Pattern q = d_syms[d_starts[q] .. d_starts[q + 1]); nsyms = d_starts[npat], by value (npat = 0 needs nsyms = 0:
 * d_result_start[0] = 0 and d_total = {0, 0, 0, 0}).  d_total[0] = the results in all, d_total[1] = 1 when they exceed `capacity`;
 * d_result_start and d_total[0] are exact whatever the capacity.  capacity = 0: d_offset and d_cost may be NULL -- the counting
 * form.  On overflow of `capacity` only d_result_start and d_total are defined: call again with capacity = d_total[0].
 * npat * (k + 1), nsyms, cand_capacity and capacity are below 2^31, FEMTO_AMD_ERR_PARAM otherwise (so is the candidate sum of a call
 * that does not overflow).
 * HANDLES.  Both forms take the extractor, whose handle does the seeding.  On an extractor on the text path the device form is
 * enqueue-only wherever femto_amd_locate_device is (rank modes 3 / 4); rank modes 0 / 1 read back what that call reads back.  Its
 * temporaries are a work area kept with the extractor: it grows (an allocation, a device-wide wait) when a call needs more than
 * any before it, and calls on one extractor run one after another on the device whatever their streams.  An extractor on the
 * sample path (or opened with FEMTO_AMD_EXTRACT_FORCE_SAMPLES) is served too: it reads the candidate total back on `stream` and
 * takes the windows from femto_amd_extract_device through at most 128 MiB of symbols at a time, which it allocates: THIS PATH
 * ALLOCATES AND WAITS.  Range-split parts and striped handles: FEMTO_AMD_ERR_INVALID.  Multi-device handle: the host form runs on
 * replica 0, the device form returns FEMTO_AMD_ERR_INVALID.
 * READS AROUND THE SYMBOLS.  The pieces are handed to the locate chain as spans of d_syms, so the note of the device-pointer batch
 * API holds: up to 14 bytes before the first and behind the last symbol of d_syms are LOADED (never used, never written); give
 * d_syms 16 bytes of slack on either side, or align its ends to 16 bytes, if a memory checker matters.  d_syms must be 2-byte
 * aligned.
 * WHAT THE DEVICE FORM IS HANDED.  d_starts and d_syms are read on the device alone.  A pattern that breaks a bound (m <= k,
 * m > 32768), whose bounds leave [0, nsyms], or that holds a code below FEMTO_AMD_CHARACTER_OFFSET or >= FEMTO_AMD_ALPHA_SIZE has no
 * results and NO CANDIDATES (its pieces reach the locate chain as patterns that match nothing, never as empty ones); the patterns
 * beside it keep the results they have alone.  Patterns that OVERLAP in d_syms are not supported. */
int femto_amd_hamming_device(femto_amd_extractor_t* ex, int64_t npat, int64_t nsyms, const uint16_t* d_syms,
                             const int64_t* d_starts /* npat + 1 */, int k, int64_t cand_capacity, int64_t capacity,
                             int64_t* d_result_start /* npat + 1 */, int64_t* d_offset, int32_t* d_cost, int64_t* d_total /* 4 */,
                             void* stream);
/* Host form (blocking): pattern i = the plen[i] symbols of `syms` that follow those of pattern i - 1 (pageable host arrays).  A
 * femto_amd_count_device of the pieces sizes the candidate buffer; then a counting pass (capacity 0) sizes the filling pass, so the
 * memory follows the results, not the candidates.  Every array of the result is malloc()ed by the callee and released by
 * femto_amd_hamming_free: result_start[npat + 1]; offset, cost [total] (NULL when total = 0); candidates = d_total[2].  A pattern
 * that breaks a bound or holds a code outside [5, 261): FEMTO_AMD_ERR_PARAM.  2^31 candidates or more: FEMTO_AMD_ERR_FULL. */
typedef struct femto_amd_hamming_result {
  int64_t npat;
  int64_t total;
  int64_t candidates;
  int64_t* result_start;
  int64_t* offset;
  int32_t* cost;
} femto_amd_hamming_result_t;
int femto_amd_hamming(femto_amd_extractor_t* ex, int64_t npat, const int32_t* plen, const uint16_t* syms, int k,
                      femto_amd_hamming_result_t* out);
void femto_amd_hamming_free(femto_amd_hamming_result_t* out);

/* ---- occurrences within k edits, by exact seeds: at which text offsets does a string within Levenshtein distance k of the pattern
 * start?  The question of femto_amd_edit (substitutions, insertions, deletions, each of cost 1) for any k up to 31, answered as
 * OFFSETS with a cost and a length rather than as strings with row ranges, and without enumerating a string: the seeds are those of
 * femto_amd_hamming, and every located piece is extended with edits to its right and to its left (femto_amd/leven/leven.hip;
 * DESIGN.md "Occurrences within k edits") ----
 * THE QUESTION.  T is the prepared text of "extraction" above (each document's bytes + 5 followed by SEOF, not cyclic).  A pattern
 * is m alpha codes, BYTE CHARACTERS ONLY (FEMTO_AMD_CHARACTER_OFFSET <= code < FEMTO_AMD_ALPHA_SIZE).  Offset p is an occurrence
 * when some substring T[p .. e), p < e <= total_length, consists of byte characters only (it never contains SEOF, so it never runs
 * over a document's end) and has Levenshtein distance <= k to the pattern.  Its result is (offset p, cost c, length L): c = the
 * smallest such distance over all e, L = the smallest e - p that reaches c.  A pattern character that the text lacks costs one
 * wherever it stands, substituted or deleted.  No result is the empty string.
 * EVERY OFFSET IS LISTED, not only the local minima: a clean hit at p brings p - k .. p + k with it (where the text allows), at
 * costs that rise by one per step.  A caller that wants one result per placement keeps the minima, as the caller of femto_amd_edit
 * drops nested ranges.
 * ORDER.  Patterns stand in batch order; pattern q's results are entries d_result_start[q] .. d_result_start[q + 1] - 1, offsets
 * ascending; an offset appears once per pattern.
 * BOUNDS.  0 <= k <= 31; k < m <= 32768: no piece is empty (k <= 31 keeps the cost in five bits of the de-duplication key and
 * length - (m - k) in six).
 * WHAT FOLLOWS.  k = 0 gives exactly the offsets of femto_amd_locate_device, with cost 0 and length m.  Every femto_amd_hamming
 * result (p, c) is a result here with cost <= c.  For k <= 2 and every result (p, c, L): the string T[p .. p + L) is one of
 * femto_amd_edit's strings for that pattern, with cost c; and every located offset o of a femto_amd_edit string of cost c is a
 * result here with cost <= c.
 * PIECES AND CANDIDATES are femto_amd_hamming's: piece j = [j m / (k + 1), (j + 1) m / (k + 1)), and the candidates are the sum,
 * over all pieces of all served patterns, of last - first + 1 as femto_amd_count_device returns it for the piece.  Every candidate
 * gives RAW RECORDS -- one for every number of text symbols in front of its piece that stays within k -- and several candidates
 * may reach one offset: the raw records are sorted by (pattern, offset, cost, length) and the first of each (pattern, offset) is
 * the result.  `cand_capacity` bounds the candidates, `capacity` the RAW records (as for femto_amd_edit_device).
 * d_total, five words:  [0] distinct results (defined only without overflow);  [1] 1 when the raw records exceed `capacity`;
 * [2] raw records, exact whatever the capacity;  [3] candidates;  [4] 1 when the candidates exceed cand_capacity: then only [3]
 * and [4] are defined -- call again with cand_capacity = d_total[3].
 * DEVICE FORM.  Pattern q = d_syms[d_starts[q] .. d_starts[q + 1]); nsyms = d_starts[npat], by value (npat = 0 needs nsyms = 0:
 * d_result_start[0] = 0 and d_total all zero).  capacity = 0: d_offset, d_cost and d_length may be NULL -- the counting form; it
 * leaves d_result_start as it is.  On overflow of `capacity` only d_total is defined: call again with capacity = d_total[2].
 * Slots behind the results are not written.  npat * (k + 1), nsyms, cand_capacity and capacity are below 2^31,
 * FEMTO_AMD_ERR_PARAM otherwise; bad arguments are refused before any device work.
 * HANDLES, READS AROUND THE SYMBOLS and WHAT THE DEVICE FORM IS HANDED are word for word femto_amd_hamming_device's, with
 * 0 <= k <= 31: enqueue-only on an extractor on the text path wherever femto_amd_locate_device is, a work area of its own kept
 * with the extractor (calls on one extractor run one after another on the device whatever their streams); range-split parts and
 * striped handles FEMTO_AMD_ERR_INVALID; multi-device handle: the host form runs on replica 0, the device form returns
 * FEMTO_AMD_ERR_INVALID; a pattern that breaks a bound, whose bounds leave [0, nsyms] or that holds a code outside [5, 261) has
 * no results and NO CANDIDATES, and the patterns beside it keep the results they have alone.  An extractor on the sample path
 * (or opened with FEMTO_AMD_EXTRACT_FORCE_SAMPLES) is served too: it reads the candidate total back on `stream` and takes a window
 * [o - b - k, o - b + m + k) around every candidate (piece start b at offset o), clipped to the text, from
 * femto_amd_extract_device through at most 128 MiB of symbols at a time, which it allocates: THIS PATH IS SLOW, ALLOCATES AND WAITS. */
int femto_amd_leven_device(femto_amd_extractor_t* ex, int64_t npat, int64_t nsyms, const uint16_t* d_syms,
                           const int64_t* d_starts /* npat + 1 */, int k, int64_t cand_capacity, int64_t capacity,
                           int64_t* d_result_start /* npat + 1 */, int64_t* d_offset, int32_t* d_cost, int32_t* d_length,
                           int64_t* d_total /* 5 */, void* stream);
/* Host form (blocking): pattern i = the plen[i] symbols of `syms` that follow those of pattern i - 1 (pageable host arrays).  A
 * femto_amd_count_device of the pieces sizes the candidate buffer; then a counting pass (capacity 0) sizes the raw records of the
 * filling pass.  Every array of the result is malloc()ed by the callee and released by femto_amd_leven_free:
 * result_start[npat + 1]; offset, cost, length [total] (NULL when total = 0); candidates = d_total[3], raw = d_total[2].  A pattern
 * that breaks a bound or holds a code outside [5, 261): FEMTO_AMD_ERR_PARAM.  2^31 candidates or raw records or more:
 * FEMTO_AMD_ERR_FULL. */
typedef struct femto_amd_leven_result {
  int64_t npat;
  int64_t total;
  int64_t candidates;
  int64_t raw;
  int64_t* result_start;
  int64_t* offset;
  int32_t* cost;
  int32_t* length;
} femto_amd_leven_result_t;
int femto_amd_leven(femto_amd_extractor_t* ex, int64_t npat, const int32_t* plen, const uint16_t* syms, int k,
                    femto_amd_leven_result_t* out);
void femto_amd_leven_free(femto_amd_leven_result_t* out);

/* ---- leaf requests (the reference's block_request interface, src/main/index.h:300-394) ---- */
/* For rows[i] (global row numbers, host memory): ch_out = L[row] (BLOCK_REQUEST_CHAR),
 * occ_out = Occ-in-block(L[row] or ch_in[i], row) (BLOCK_REQUEST_OCCS; ch_in==NULL -> use L[row]),
 * off_out = mark offset or -1 (BLOCK_REQUEST_LOCATION).  Any output pointer may be NULL. */
int femto_amd_block_requests(femto_amd_index_t* ix, int64_t n, const int64_t* rows, const uint16_t* ch_in,
                             uint16_t* ch_out, int32_t* occ_out, int64_t* off_out);

/* One LF^-1 step per row (do_forward_query, src/main/server.c:2424; HDR_BSEARCH_C|HDR_BSEARCH_BLOCK_OCCS|
 * HDR_FORWARD then BLOCK_REQUEST_ROW|BLOCK_REQUEST_LOCATION, src/main/index.c:1698,1915): ch_out = first
 * character of the row, row_out = the row whose LF step leads here (-1 when ch <= SEOF), off_out = that
 * row's mark offset or -1.  Exercises bseq_select / wtree_select (src/main/wtree.c:770,1150) on the GPU. */
int femto_amd_forward_steps(femto_amd_index_t* ix, int64_t n, const int64_t* rows, uint16_t* ch_out,
                            int64_t* row_out, int64_t* off_out);

/* ---- range-split index (BASELINE.json configs[4]) ------------------------------
 * The reference scales an index past memory by block: a row belongs to data block row / block_size
 * (bsearch_block_rows, src/main/index.c:1613-1617) and blocks are faulted from disk one by one through
 * its block cache.  On one MI355X node the blocks are partitioned over the GPUs and a "block fault" is a plain
 * load: part p keeps the segment lines and block images of blocks [nblocks*p/nparts,
 * nblocks*(p+1)/nparts) in its own HBM, maps the other parts' slices into its address space
 * (hipIpcOpenMemHandle across processes, peer access inside one process) and the SAME lane kernels
 * read remote lines over xGMI.  The small per-bucket tables (Occ bases, tree shapes, block
 * directories) are replicated.  Every part answers any query; batches are sharded as with a
 * replicated index.
 *
 *   femto_amd_open_split(path, dev, part, nparts, &ix)      on every part
 *   femto_amd_split_export(ix, blob)                         128-byte blob, send to all other parts
 *   femto_amd_split_attach(ix, p, blob_of_p)                 for every other part p   (other process)
 *   femto_amd_split_attach_local(ix, handle_of_p)            ... or, same process
 *   femto_amd_split_commit(ix)                               then count/locate as usual
 * A part must stay open while any other part that attached it is in use.  Only the lane kernels
 * (mode 1) run on a range-split index; femto_amd_forward_steps is not available. */
int femto_amd_open_split(const char* index_path, int device, int part, int nparts, femto_amd_index_t** out);
int femto_amd_split_export(femto_amd_index_t* ix, void* blob128);
int femto_amd_split_attach(femto_amd_index_t* ix, int part, const void* blob128);
int femto_amd_split_attach_local(femto_amd_index_t* ix, femto_amd_index_t* owner);
int femto_amd_split_commit(femto_amd_index_t* ix);
/* bytes of this part's own slices (segment lines, block images) */
int femto_amd_split_info(const femto_amd_index_t* ix, int* part, int* nparts, int64_t* seg_bytes, int64_t* image_bytes);

/* ---- regular expressions and automata (do_regexp_query src/main/server.c:1656, nfa.c, compile_regexp.c) ----
 * The reference searches a regular expression by simulating an EPSILON-FREE automaton of the REVERSED pattern backwards over
 * the index (do_regexp_query): femto_amd_nfa_t is that automaton, field for field the reference's nfa_description_t
 * (src/main/nfa.h:62-88) with the arrays flattened -- node i's transitions are entries trans_start[i] .. trans_start[i+1]-1 of
 * trans_char[] (alpha codes, byte + 5) / trans_dest[]; is_start / is_final are the two bit sets; the four costs are
 * regexp_settings_t (src/main/index_types.h:147-162: cost_bound = largest allowed total cost + 1, 1 = exact matching).
 *
 * femto_amd_nfa_search_batch replaces setup_regexp_query_take_nfa (src/main/server.h:838) + do_regexp_query for nq automata at
 * once, each searched by one GPU workgroup (regexp_search.hip): for automaton q the results are entries
 * result_start[q] .. result_start[q+1]-1 of first_out / last_out (row range of a matched string: locate its rows with
 * femto_amd_parallel_locate_range), len_out (match_len: symbols of the matched string) and cost_out (errors), in the order
 * of the reference's sorted result list (regexp_result_list_sort, server.c:1528: first ascending, last descending, equal
 * ranges and ranges inside another result dropped) -- IDENTICAL to the reference's list for the same automaton, quirks
 * included (a range with a final state alive is a result and is NOT extended; a pending range reached again is merged).
 * status_out[q] (may be NULL): 0, FEMTO_AMD_ERR_OVERWORKED (more than MAX_REGEXP_ITERATIONS = 10^6 steps, server.c:40,1821:
 * the reference returns ERR_OVERWORKED and no results) or FEMTO_AMD_ERR_FULL (more pending ranges than option
 * "regexp_stack_cap", default 2^18, at most 2^22; the reference has no such bound -- it would run on to ERR_OVERWORKED).  The out arrays hold max_results entries for ALL
 * automata together; *n_out = results in total; max_results == 0 only counts (result_start[] and *n_out are filled, the
 * other out arrays may be NULL); more results than max_results is FEMTO_AMD_ERR_FULL with *n_out = the exact number
 * to call again with (raw result ranges are buffered by the library itself; only when even its buffer -- up to half of the
 * free HBM, 16 GB at most -- cannot hold them is *n_out the RAW count: an upper bound, before equal and nested ranges are dropped).  Limits: 2048 nodes, 2^22 transitions per
 * automaton, costs and cost_bound 1..255 (errors are counted in one byte, nfa.h:74-76). */
typedef struct femto_amd_nfa {
  int32_t num_nodes;
  int32_t num_transitions;
  const int32_t* trans_start;   /* [num_nodes + 1] */
  const int32_t* trans_char;    /* [num_transitions] alpha codes */
  const int32_t* trans_dest;    /* [num_transitions] */
  const uint8_t* is_start;      /* [num_nodes] */
  const uint8_t* is_final;      /* [num_nodes] */
  int32_t cost_bound, subst_cost, delete_cost, insert_cost;
} femto_amd_nfa_t;
int femto_amd_nfa_search_batch(femto_amd_index_t* ix, int64_t nq, const femto_amd_nfa_t* nfas, int64_t max_results,
                               int64_t* result_start /* nq + 1 */, int64_t* first_out, int64_t* last_out, int32_t* len_out,
                               int32_t* cost_out, int32_t* status_out, int64_t* n_out);
/* What the handle's last automaton batch did (the reference keeps many do_regexp_query state machines in flight,
 * src/main/server.c:3969-4001; here concurrent callers' batches share the GPU's workgroups, each kernel giving up its
 * workgroups beyond a fair share between automata): out8 = { automata, workgroups launched, entries popped in all, ... by the
 * longest search, busy workgroup-seconds, the span of the search passes in seconds (both on the device's wall clock),
 * occupancy = busy / (span x workgroups), seconds the longest search waited before a workgroup took it }.
 * ix == NULL: the calling thread's own last batch. */
int femto_amd_nfa_stats(femto_amd_index_t* ix, double* out8);
/* Pattern text -> automaton.  Pattern language: femto's own (src/main/QUERY_FORMAT.txt), restated token rule by token rule
 * and production by production from src/main/posix.flex.l and src/main/posix.bison.y (femto_amd/csrc/query_parser.hpp names
 * the corners): literal bytes, `.`, `[a-z]` / `[^...]`, `( )`, `|`, one of `*` `+` `?` `{m}` `{m,}` `{m,n}` per term, backslash
 * escapes (\n \t \xNN, \x-NN for the codes below the bytes), "double" and 'single' quotes, `{x 00 01}` hex strings, `#`
 * comments, runs of three or more letters as one term; unescaped whitespace separates terms and is ignored; a leading
 * APPROX [max_cost[:subst[:delete[:insert]]]] sets the costs.  The boolean operators (AND OR NOT THEN WITHIN: document-level
 * result sets) are recognised and refused here; femto_amd_bquery_compile, below, reads them.  The automaton is the position (Glushkov) automaton of the reversed pattern.
 * (The reference's generated front end -- flex/bison, then compile_regexp.c -- cannot be built in this image; search parity
 * is pinned at the automaton: the same femto_amd_nfa_t goes to the genuine do_regexp_query and to
 * femto_amd_nfa_search_batch; the grammar is pinned by the known answers of src/main/query_planning_test.c and by the
 * query set of src/test/test.pl.)  APPROX costs are validated as compile_regexp_from_ast does (compile_regexp.c:673-685:
 * three substitutions or insertions are refused).  Limits: 2^20 bytes of pattern text, parentheses nested 256 deep,
 * repeat counts <= 4096, 4096 Thompson states: beyond them FEMTO_AMD_ERR_PARAM, never a crash. */
typedef struct femto_amd_regexp femto_amd_regexp_t;
int femto_amd_regexp_compile(const uint8_t* regex, int64_t regex_len, int max_cost, int subst_cost, int delete_cost,
                             int insert_cost, femto_amd_regexp_t** out);
const femto_amd_nfa_t* femto_amd_regexp_nfa(const femto_amd_regexp_t* r);   /* valid until femto_amd_regexp_free */
/* A whole femto_search query, prepared as src/main_cc/search_tool.cc:716-751 prepares it: parse_string, then streamline_query
 * (src/main/query_planning.c:24: optional parts at either end of the pattern are dropped and repeats there trimmed to their
 * minimum -- "a*(bc|d)+" is searched as "(bc|d)"), simplify_query (ast.c:1239: a query without alternatives is ONE string),
 * and, with FEMTO_AMD_QUERY_ICASE, icase_ast (ast.c:556; femto_search --icase).  An APPROX prefix in the text sets the costs. */
#define FEMTO_AMD_QUERY_ICASE 1
#define FEMTO_AMD_QUERY_NO_STREAMLINE 2
int femto_amd_query_compile(const uint8_t* query, int64_t query_len, int flags, femto_amd_regexp_t** out);
/* 1 when the prepared query is one plain string (search it with femto_amd_count_flat / _locate_flat as femto_search runs a
 * string query, src/main/server.c:713): *syms / *n its alpha codes, owned by r; 0 otherwise */
int femto_amd_regexp_literal(const femto_amd_regexp_t* r, const uint16_t** syms, int64_t* n);
/* the prepared query printed back as ast_to_string(ast, 0, 1) prints it (src/main/ast.c:1122; femto_search --json "pattern") */
const char* femto_amd_regexp_echo(const femto_amd_regexp_t* r);
/* test hook for the known answers of src/main/query_planning_test.c and for tests/golden/query_ast_golden.json (the genuine
 * streamline_query / simplify_query / icase_ast / ast_to_string run on the tree this parser produced): parse, then flags bit 0
 * streamline, bit 1 simplify, bit 2 icase; print back with (1) or without (0) quotes into out[cap] -- usequotes 2: the parsed
 * tree in the text form oracle/ref_tool.c `ast` reads.  Returns the length, -1 on a syntax error or a buffer too small */
int femto_amd_query_echo(const uint8_t* query, int64_t query_len, int flags, int usequotes, char* out, int64_t cap);
void femto_amd_regexp_free(femto_amd_regexp_t* r);
/* compile + search, a batch of patterns with the same costs (max_cost = 0, costs 1: exact) */
int femto_amd_regexp_search_batch(femto_amd_index_t* ix, int64_t nq, const uint8_t* const* regex, const int64_t* regex_len,
                                  int max_cost, int subst_cost, int delete_cost, int insert_cost, int64_t max_results,
                                  int64_t* result_start, int64_t* first_out, int64_t* last_out, int32_t* len_out,
                                  int32_t* cost_out, int32_t* status_out, int64_t* n_out);
/* one pattern; a search that ends OVERWORKED / FULL returns that code */
int femto_amd_regexp_search(femto_amd_index_t* ix, const uint8_t* regex, int64_t regex_len, int64_t max_results,
                            int64_t* first_out, int64_t* last_out, int32_t* len_out, int64_t* n_out);
int femto_amd_regexp_search_approx(femto_amd_index_t* ix, const uint8_t* regex, int64_t regex_len, int max_cost,
                                   int subst_cost, int delete_cost, int insert_cost, int64_t max_results,
                                   int64_t* first_out, int64_t* last_out, int32_t* len_out, int32_t* cost_out,
                                   int64_t* n_out);
/* test hook: does the automaton built from `regex` accept exactly the byte string s?  1 yes, 0 no, -1 syntax error */
int femto_amd_regexp_match(const uint8_t* regex, int64_t regex_len, const uint8_t* s, int64_t len);

/* ---- boolean queries: AND OR NOT THEN WITHIN of the query language (boolean_exp, src/main/posix.bison.y:122-135;
 * setup_generic_boolean_query, src/main/server.c:5369) ----
 * OPT-IN.  femto_amd_query_compile still refuses the operators; femto_amd_bquery_compile reads them:
 *     exp := exp op rest | rest                 left-associative, no precedence: "a AND b OR c NOT d" is ((a AND b) OR c) NOT d
 *     rest := term | '(' exp op rest ')'        a group that holds an operator takes no repeat operator
 * op is AND OR NOT THEN [n] WITHIN n, upper or lower case, followed by whitespace; THEN without a number has the distance
 * INT_MAX.  A term is a query of the language above (APPROX may lead it) and goes through femto_amd_query_compile's whole
 * pipeline on its own (the reference streamlines, simplifies and --icase's into boolean nodes).  femto_amd/bquery/bquery_parser.hpp
 * names the corners.  `flags` are femto_amd_query_compile's.
 * TYPES.  A list is documents (FEMTO_AMD_BQUERY_DOCUMENTS) or (document, offset in document) pairs (FEMTO_AMD_BQUERY_PAIRS).  A term
 * under AND / OR / NOT is listed as documents, under THEN / WITHIN as pairs; AND and NOT take either kind on either side and
 * yield documents; OR needs the same kind on both sides and yields it; THEN and WITHIN need pairs on both sides and yield pairs.
 * A tree the reference fails with ERR_PARAM while it runs -- "(a THEN b) OR c" -- is refused at compile time: FEMTO_AMD_ERR_PARAM,
 * the message names the operator and its byte offset.  The result type is the root's (a query that is one term: documents).
 * femto_amd_bquery_node: node i of the tree in POSTFIX order (both children stand before their parent, the root is the last
 * node): *op = FEMTO_AMD_BQUERY_LEAF or the operator, *distance (THEN / WITHIN), *left / *right = node numbers (-1 for a leaf),
 * *leaf = the compiled term (NULL for an operator; owned by the query).  Any output may be NULL.
 * femto_amd_bquery_echo: ast_to_string(ast, 0, 1) (src/main/ast.c:1078-1110: left, " AND " / " THEN 20 " ..., right; no
 * parentheses) -- femto_search --json's "pattern".
 * SEMANTICS of femto_amd_bquery_run_batch (blocking; host arrays in, malloc()ed packed results out, as femto_amd_docpos): query k's
 * result is entries [res_starts[k], res_starts[k + 1]) of *res_doc / *res_off, ascending; res_type[k] is its type; the *res_off
 * entries of a document-typed result are 0.  *res_doc / *res_off are NULL when *total = res_starts[nq] is 0; the caller free()s.
 *   - A node's operands are the WHOLE lists of its children.  The reference evaluates in chunks of 2^20 results
 *     (src/main_cc/search_tool.cc:799-803 fixes the chunk size of a boolean query) and, beyond one chunk, its results depend on
 *     where the chunks end; up to one chunk the two agree.
 *   - AND, OR, NOT are femto_amd_docset_device's, THEN, WITHIN and OR of pairs femto_amd_docpos_device's, with their semantics
 *     as stated above, the "written once" departure of WITHIN included.
 *   - AND / NOT over a pair-typed operand use each of its documents ONCE (femto_amd_docpos_documents_device).  A DEPARTURE: the
 *     reference's intersectResults / subtractResults step through the pairs entry by entry, so a document that stands k times on
 *     either side is matched k times: its writer fails with ERR_PARAM as soon as a document would be written twice
 *     (append_document_internal, results.c:145), and NOT keeps a document that stands more often on the left than on the right.
 *   - THE LISTS DESCRIBE THE ROWS THAT WERE LOCATED, as with femto_amd_doclist: with a max_occs_each clamp a term's list is made
 *     of the rows parallel_locate returns for it (do_locate_query's clamp; for a term that is an automaton: its result ranges in
 *     order until max_occs_each rows are in, the first range clamped as a pattern's is), and a result is the operators applied to those.
 *   - A row that an automaton's result ranges hold twice (APPROX, alternation) is listed once (the reference's sort_dedup).
 * COST.  All terms that are strings are counted by one femto_amd_count_device, all automata searched by one
 * femto_amd_nfa_search_batch, all rows walked by one femto_amd_locate_walk_device and listed by one femto_amd_doclist_device;
 * then the nodes of one height of ALL trees are one femto_amd_docset_device and one femto_amd_docpos_device call (plus one
 * femto_amd_docpos_documents_device where an AND / NOT reads positional results).  No result is longer than the rows of the terms
 * below it, so every level's buffers are sized from the terms' row counts: the host waits for the device TWICE per batch -- for
 * the terms' row counts and for the result starts -- and never per level (and once per automaton search, which returns to
 * the host by its interface).  2^31 or more located rows in one call: FEMTO_AMD_ERR_PARAM (split the batch).
 * A term whose automaton search ends OVERWORKED / FULL fails the batch with that code.
 * Handles: as for femto_amd_doclist (range-split parts and striped handles FEMTO_AMD_ERR_INVALID; multi-device handle: replica 0). */
#define FEMTO_AMD_BQUERY_LEAF 0
#define FEMTO_AMD_BQUERY_AND 1
#define FEMTO_AMD_BQUERY_OR 2
#define FEMTO_AMD_BQUERY_NOT 3
#define FEMTO_AMD_BQUERY_THEN 4
#define FEMTO_AMD_BQUERY_WITHIN 5
#define FEMTO_AMD_BQUERY_DOCUMENTS 0
#define FEMTO_AMD_BQUERY_PAIRS 1
typedef struct femto_amd_bquery femto_amd_bquery_t;
int femto_amd_bquery_compile(const uint8_t* query, int64_t query_len, int flags, femto_amd_bquery_t** out);
int femto_amd_bquery_info(const femto_amd_bquery_t* q, int* nodes, int* leaves, int* result_type);
int femto_amd_bquery_node(const femto_amd_bquery_t* q, int i, int* op, int* distance, int* left, int* right,
                          const femto_amd_regexp_t** leaf);
const char* femto_amd_bquery_echo(const femto_amd_bquery_t* q);
void femto_amd_bquery_free(femto_amd_bquery_t* q);
int femto_amd_bquery_run_batch(femto_amd_index_t* ix, int64_t nq, const femto_amd_bquery_t* const* queries, int max_occs_each,
                               int64_t* res_starts /* nq + 1 */, int32_t* res_type /* nq */, int64_t** res_doc, int64_t** res_off,
                               int64_t* total);

/* ---- several GPUs of one node ----------------------------------------------------------------------------------------
 * Queries are independent (each string_query_t is its own state machine, src/main/server.c:3969-4001), so a batch shards
 * with no exchange during the search.
 *
 * One process, several GPUs -- what the C caller of parallel_count (src/main/femto.c:275) needs: femto_amd_open_multi
 * opens the index on every listed device (replicated) and returns an ordinary handle; the HOST-pointer batch calls
 * (femto_amd_parallel_count / _parallel_locate / _count_flat / _locate_flat / _locate_flat_alloc /
 * _parallel_locate_range) then split the batch into contiguous shards, one host thread per GPU, and every GPU returns
 * its shard straight into the caller's arrays over its own PCIe link -- no gather at all.  Device-pointer calls are not
 * available on such a handle (FEMTO_AMD_ERR_INVALID).  INTEGRATION.md: the shim opens one when FEMTO_AMD_DEVICES lists
 * more than one device. */
int femto_amd_open_multi(const char* index_path, int ndev, const int* devices, femto_amd_index_t** out);
/* The same handle for an index LARGER than one GPU's HBM (BASELINE configs[4]; the reference partitions by block,
 * bsearch_block_rows src/main/index.c:1613-1617): every big array -- block images, segment lines, packed / two-level /
 * per-character lines, level table, suffix arrays, text -- is ONE address range whose pages live in the HBM of all the
 * listed GPUs in equal contiguous stripes (HIP virtual memory management: hipMemCreate per GPU, one hipMemMap'ed
 * range, access granted to every GPU), the small tables are copied to every GPU.  The kernels are unchanged: a line in
 * another GPU's stripe is an ordinary load that travels over xGMI -- the packed fast paths, unlike
 * femto_amd_open_split's wavelet-path kernels, keep working.  Batches shard over the GPUs as with femto_amd_open_multi. */
int femto_amd_open_multi_striped(const char* index_path, int ndev, const int* devices, femto_amd_index_t** out);
int femto_amd_device_count(const femto_amd_index_t* ix);
/* One process per GPU, results resident on the devices: the only exchange is the final gather of the shards' results
 * to one rank -- a grouped batch of ncclSend / ncclRecv over xGMI (RCCL is loaded on first use, it is not a link-time
 * dependency).  Bootstrap as with NCCL: one rank makes the 128-byte id, every rank passes it to femto_amd_comm_init
 * (any transport; bench.py --gather native broadcasts it through torch.distributed).  femto_amd_comm_gather enqueues on
 * `stream`: rank r's bytes_per_rank bytes arrive at d_recv + r * bytes_per_rank on `root` (d_recv is ignored elsewhere). */
int femto_amd_comm_unique_id(void* id128);
int femto_amd_comm_init(femto_amd_index_t* ix, const void* id128, int nranks, int rank);
int femto_amd_comm_gather(femto_amd_index_t* ix, const void* d_send, void* d_recv, int64_t bytes_per_rank, int root, void* stream);
/* the communicator's own view: ranks it spans and this handle's rank in it (ncclCommCount / ncclCommUserRank) */
int femto_amd_comm_info(femto_amd_index_t* ix, int* nranks, int* rank);

/* A striped index shared between PROCESSES (one process per GPU; BASELINE.json configs[4], "index range-split across 8
 * GPUs"; the owner of a stripe is position / chunk as the owner of a row is row / block_size in bsearch_block_rows,
 * src/main/index.c:1613).  The process that called femto_amd_open_multi_striped serves `nclients` other processes: every
 * physical stripe travels as a POSIX file descriptor over the Unix-domain socket `socket_path` (SCM_RIGHTS), with a
 * description of the handle.  femto_amd_open_striped_client (index_path: the same index, for its header and document
 * table) maps the stripes at the builder's addresses, copies the small tables to `device` and returns an ordinary
 * single-GPU handle -- every kernel family and fast path, remote lines over xGMI; it waits up to timeout_s seconds for the
 * builder's socket.  femto_amd_multi_child returns replica i of a multi-device handle (a borrowed single-GPU handle, valid
 * until the parent is closed): replica 0 of a striped handle is the builder's own. */
int femto_amd_striped_serve(femto_amd_index_t* ix, const char* socket_path, int nclients);
int femto_amd_open_striped_client(const char* index_path, const char* socket_path, int device, int timeout_s, femto_amd_index_t** out);
int femto_amd_multi_child(femto_amd_index_t* ix, int i, femto_amd_index_t** child);

/* ---- patterns as keys (device pointers) ---------------------------------------------------------------------------------
 * A pattern of at most max_syms symbols whose characters all occur in the text fits ONE 64-bit word: `bits`-bit fields, the
 * pattern's LAST symbol in the top field, field = field_of_alpha[alpha code] (1 + the character's dense code: its rank among the
 * text's characters -- by character value on small alphabets, by falling frequency behind the characters <= SEOF on byte
 * alphabets: take the table, do not derive it), 0 = end of pattern.  femto_amd_key_format reports bits / max_syms (3 bits, 21 symbols for DNA; 7 bits, 9
 * symbols for a 96-character text) and the field table; femto_amd_pack_keys_device packs a (plen, pats, starts) batch that
 * is already in HBM (*d_bad = patterns no key describes: they get key 0 = the empty pattern; such a batch belongs to the
 * symbol entry points).  femto_amd_locate_keys_device is femto_amd_count_device / femto_amd_locate_device on keys: the
 * same search (parallel_count / parallel_locate, src/main/femto.c:275,331), bit-identical results, 8 bytes of input per
 * pattern instead of 12 + 2 per symbol, and -- d_ranges32 != NULL, an index of fewer than 2^31 - 1 rows -- the ranges as
 * int32 (first, last) pairs instead of two int64 arrays.  d_noccs == NULL: count only (d_out_starts / d_offsets / d_total
 * unused).  Enqueue-only, like the calls it mirrors. */
int femto_amd_key_format(const femto_amd_index_t* ix, int* bits, int* max_syms, uint8_t* field_of_alpha /* [261] or NULL */);
/* An identity of the key fields of this handle (a hash of `bits` and field_of_alpha): keys are only meaningful to a handle -- and a
 * library build -- that reports the SAME id.  A caller that packs keys itself, caches them, or ships them to another process
 * compares ids first: the fields follow the handle's dense codes, which differ between indexes and have changed between library
 * versions (byte alphabets: by falling frequency since round 5); a key of another table searches for another string, silently. */
int femto_amd_key_table_id(const femto_amd_index_t* ix, uint64_t* id);
int femto_amd_pack_keys_device(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen, const uint16_t* d_pats,
                               const int64_t* d_starts, uint64_t* d_keys, int64_t* d_bad, void* stream);
int femto_amd_locate_keys_device(femto_amd_index_t* ix, int64_t npats, const uint64_t* d_keys, int max_occs_each,
                                 int32_t* d_ranges32 /* [2 * npats] or NULL */, int64_t* d_first, int64_t* d_last,
                                 int32_t* d_noccs, int64_t* d_out_starts /* npats + 1 */, int64_t* d_offsets,
                                 int64_t offsets_capacity, int64_t* d_total /* 2 */, void* stream);

/* The match counts of a batch in the form a result gather sends ("one RCCL collective for results";
 * parallel_count's last == NULL form, src/main/femto.c:313-318, narrowed): d_counts8[i] = min(last[i] - first[i] + 1, 255),
 * 0 when there is no match; every pattern with 255 matches or more is appended to d_big as a pair (pattern index, count),
 * in no particular order, and *d_big_n receives how many there are (pairs beyond big_capacity are not written).  Lossless;
 * one byte per pattern on the links.  Enqueue-only, device pointers. */
int femto_amd_pack_counts_device(femto_amd_index_t* ix, int64_t npats, const int64_t* d_first, const int64_t* d_last,
                                 uint8_t* d_counts8, int64_t* d_big, int64_t big_capacity, int64_t* d_big_n, void* stream);

/* ---- options of an open handle ---------------------------------------------------------------------------------------------
 * What is derived at open, and how much HBM it may take, decided by the CALLER: fill the struct with femto_amd_options_init
 * (every field "auto") and set what matters.  -1 (auto) = the rule described with each field; the environment variables
 * named in brackets are read ONLY for fields left on auto -- they are test overrides, not the configuration interface.
 * DESIGN.md 3 has the measured table level_table_syms -> bytes -> ms per step a deployer picks a budget from. */
#define FEMTO_AMD_BUDGET_ALL (-2)
typedef struct femto_amd_options {
  uint32_t struct_size;          /* sizeof(femto_amd_options_t), set by femto_amd_options_init: versions the struct */
  int32_t rank_mode;             /* -1: the fastest that applies | 0 raw | 1 lane | 3 pack | 4 pack2   [FEMTO_AMD_RANK_MODE] */
  int64_t hbm_budget_bytes;      /* bytes this handle may HOLD in all (femto_amd_structures[13]): the optional structures are
                                  * declined (identical results on the slower path) once it is spent; the level table takes
                                  * what the lines, marks and rank units leave.  -1 (auto): the DEFAULT BOUND
                                  * min(free HBM / 4, max(8 x indexed text bytes, 2 GiB)) -- 8.6 GB for a 1 GiB text, where a
                                  * random 20-mer costs ~3 memory requests instead of ~1.3.  FEMTO_AMD_BUDGET_ALL (-2): whatever
                                  * is free on the device (dense suffix arrays, deepest tables: the benchmark's setting; DESIGN.md
                                  * 3 has bytes -> patterns/s).                                        [FEMTO_AMD_HBM_BUDGET] */
  int32_t packed_lines;          /* 0: skip mode 3's lines                                                [FEMTO_AMD_PACK] */
  int32_t two_level_lines;       /* 0: skip mode 4's lines | 1: build them for <= 8 characters too        [FEMTO_AMD_PACK2] */
  int32_t char_rank_lines;       /* 0: skip the per-character rank lines of byte alphabets                [FEMTO_AMD_IND] */
  int32_t text;                  /* 0: skip text + inverse suffix array (no text tail)                    [FEMTO_AMD_TEXT] */
  int32_t dense_arrays;          /* 0: sampled suffix / inverse suffix arrays only                        [FEMTO_AMD_DENSE] */
  int32_t mark_every;            /* derived marks every n-th text position, 0 = femto's own marks; auto 5 [FEMTO_AMD_MARK_EVERY] */
  int32_t level_table;           /* 0: no level table                                                     [FEMTO_AMD_KTAB] */
  int32_t level_table_syms;      /* K, the deepest level; auto: <= 4 entries per row within the budget   [FEMTO_AMD_KTAB_SYMS] */
  int64_t level_table_bytes;     /* cap of the level table; auto: a quarter (60 % for <= 1 entry per row) of the free HBM [.._KTAB_MB] */
  int32_t context_table;         /* 0: no context tables (byte alphabets)                                 [FEMTO_AMD_CTX] */
  int32_t context_syms;          /* H of the narrow table                                                 [FEMTO_AMD_CTX_SYMS] */
  int32_t context2_table;        /* 0: no wide table                                                      [FEMTO_AMD_CTX2] */
  int32_t context2_syms;         /* H2 of the wide table (<= 16)                                          [FEMTO_AMD_CTX2_SYMS] */
  int64_t context2_bytes;        /* cap of the wide table; auto: a quarter of the free HBM                [FEMTO_AMD_CTX2_MB] */
  int32_t tail_min, tail_ones, tail_rows, tail_row_cost;   /* thresholds of the text tail (direct_kernels.hip.hpp) [FEMTO_AMD_TAIL_*] */
  int32_t sort_queries;          /* 0: mode 1 does not order large batches by suffix                      [FEMTO_AMD_SORT] */
  int32_t host_threads;          /* staging threads of host-pointer batches; auto: half the hardware threads, <= 128, <= twice a cgroup CPU quota [.._HOST_THREADS] */
  int32_t host_pipeline;         /* 0: host-pointer batches are staged in one piece                       [FEMTO_AMD_HOST_PIPELINE] */
  int32_t host_keys;             /* 0: host-pointer batches travel as symbols, never as keys              [FEMTO_AMD_HOST_KEYS] */
  int32_t host_pipe_chunk_log2;  /* log2 patterns per pipeline stage; auto 20                             [FEMTO_AMD_PIPE_CHUNK_LOG2] */
  int32_t host_d2h_staged;       /* 0: located offsets return with one plain copy                         [FEMTO_AMD_D2H_STAGED] */
  int32_t rank_units;            /* the 16-byte rank units of small alphabets (ru_kernels.hip.hpp): 0 none, 1 auto, 2 plain (88 rows), 3 marked (64 rows + mark bits; auto picks them when the handle will not hold the suffix array) [FEMTO_AMD_RU] */
  int32_t marks_32bit;           /* 0: derived mark offsets stay 8 bytes; auto: 4 bytes when the index has < 2^32 rows [FEMTO_AMD_SA32] */
  int32_t context_mid_table;     /* 1: a third context table of the length half way between the other two; auto: none [FEMTO_AMD_CTXM] */
  int32_t wavelet_lines;         /* femto's OWN tables -- the block files as uploaded and its wavelet tree as segment lines (modes 0/1;
                                  * every derivation reads them, the derived layouts' kernels do not): 1 keep them in HBM | 0 release them
                                  * once the derived layouts stand; they come back, counted, for the calls that read them
                                  * (femto_amd_set_rank_mode(0/1), LOCATION leaf requests, femto_amd_forward_steps) and leave again when
                                  * they put the handle over its budget | auto: released on handles with a budget -- 1.3 GB of a 1 GiB DNA
                                  * index that then pays for rank units, marks, the suffix array  [FEMTO_AMD_WAVELET_LINES] */
} femto_amd_options_t;
void femto_amd_options_init(femto_amd_options_t* opts);
/* femto_amd_open with options (NULL = all auto = femto_amd_open) */
int femto_amd_open_opts(const char* index_path, int device, const femto_amd_options_t* opts, femto_amd_index_t** out);

/* ---- kernel family ---------------------------------------------------------------------------- */
/* Four kernel families, all bit-exact; the default at open is the fastest that applies (mode 3 for <= 8 distinct
 * characters, mode 4 for <= 256, else mode 1); FEMTO_AMD_RANK_MODE=pack|pack2|lane|raw overrides it.
 * mode 3 ("pack"): for indexes with at most 8 distinct characters (DNA) the loader derives, on the GPU, one self-contained
 *   128-byte line per 160 rows -- three bit planes of the dense character code, a "row is marked" plane, and C[ch]+Occ
 *   before the line for each character -- so that an Occ and a whole locate step each read ONE memory line
 *   (femto_amd/csrc/pack_kernels.hip.hpp).
 * mode 4 ("pack2"): 9..256 distinct characters -- a two-level 16-ary decomposition of the dense character code, one
 *   128-byte line per level (pack2_kernels.hip.hpp), plus per-character rank lines for the search steps
 *   (ind_kernels.hip.hpp) and hashed context tables of the text's H-grams (ctx_kernels.hip.hpp) when HBM allows.
 *   Modes 3 and 4 process a batch in the CALLER's order, one lane per pattern, the first steps from a level table
 *   precomputed at open (direct_kernels.hip.hpp); they also derive the full suffix array / inverse suffix array / text
 *   (HBM allowing) so that locate is one read and a long pattern's tail is compared with the text.
 * mode 1 ("lane"): one LANE per query on femto's own wavelet tree; a rank reads one 128-byte line per segment (segment +
 *   the counts before it) from tables derived at load time.  Alphabets of more than 256 characters, range-split indexes.
 * mode 0 ("raw"): one WAVEFRONT per query walking femto's own A0/A1/AP group tables and varbyte S sums with
 *   __ballot / ds_bpermute, no derived tables at all -- BASELINE.json north_star's sketch, kept as the documented
 *   reference kernel (5 % of the HBM roofline) and for indexes whose segments the derived tables cannot
 *   describe.
 * (Rounds 1-2 also carried a persistent-grid variant of mode 1 and suffix-sorted variants of modes 3/4; both measured
 * slower than what replaced them and were removed.) */
int femto_amd_set_rank_mode(femto_amd_index_t* ix, int mode);
/* Runtime switches of an open handle: "sort" (default 1: mode 1 orders large batches by pattern suffix),
 * "regexp_max_iterations" (default 10^6 = MAX_REGEXP_ITERATIONS), "regexp_stack_cap" (default 2^18). */
int femto_amd_set_option(femto_amd_index_t* ix, const char* name, int value);
/* What was derived (diagnostics; femto_amd/__init__.py pack_info() names every bit): *available bit 0 packed lines, 1 two-level lines,
 * 2 level table, 3 suffix array of every row, 4 inverse suffix array of every position, 5 per-character rank lines, 6 context table,
 * bits 8..11 / 12..16 / 24..28 the context tables' symbol counts, bit 20 rank units, bit 21 the MARKED rank units (64 rows + mark
 * bits: handles that walk to marks), bit 22 the suffix / inverse suffix arrays hold 4-byte entries (indexes of fewer than 2^32 - 1 rows). */
int femto_amd_pack_info(const femto_amd_index_t* ix, int* available, int64_t* bytes, double* build_ms, int* ktab_syms);
/* What the handle holds in HBM, in bytes -- the server's "what may a handle spend" made visible (the counterpart of
 * server_settings_t's cache sizes, src/main/server.c:3484-3602): out[0] the femto block files as uploaded, [1] packed lines,
 * [2] offsets of the derived marks, [3] rank units, [4] level table, [5] context tables, [6] per-character rank lines,
 * [7] text + suffix / inverse suffix arrays, [8] two-level lines, [9] everything derived (lane tables included),
 * [10] distance between derived marks (0: femto's own), [11] level-table depth K, [12] bytes per mark offset,
 * [14] the HBM budget in force (-1: everything that is free), [15] 1 when it is the default bound (hbm_budget_bytes auto),
 * [13] HBM the handle holds in all (every persistent allocation of the INDEX: what hbm_budget_bytes is counted against; the
 * scratch of batch calls -- patterns, results; in the host-pointer API also the staging buffers a call's scratch keeps for the
 * next call, up to ~0.4 GB pinned host + ~0.4 GB device per concurrently calling thread -- is not part of it).  n <= 16. */
int femto_amd_structures(const femto_amd_index_t* ix, int64_t* out, int n);
/* Where the LAST staged host-pointer batch call (femto_amd_count_flat / _parallel_count ... on >= 2^18 patterns) spent its
 * wall time, in ms: out8[0] staging threads packing the caller's patterns into pinned key / symbol chunks, [1] waiting for
 * a pinned input buffer, [2] enqueueing copies / kernels / events, [3] waiting for a chunk's results to arrive over PCIe,
 * [4] staging threads moving results into the caller's arrays, [5] the whole call; [6] chunks, [7] staging threads. */
int femto_amd_host_pipeline_stats(femto_amd_index_t* ix, double* out8);
/* The staging threads' packing loop on its own (no handle, no device; diagnostic): keys_out[i] = the 64-bit key of pattern i
 * (symbols flat[starts[i] .. starts[i] + plen[i]), dense[sym] = the symbol's field for sym < ndense, `bits` bits per field,
 * last symbol in the top field: what femto_amd_pack_keys_device computes on the GPU).  Returns 1 when every pattern is described
 * by its key, 0 when some pattern is not (longer than 63 / bits symbols, a symbol without a field: such a chunk travels as
 * symbols), -1 on bad arguments.  force_scalar != 0: the plain loop instead of the AVX-512 VBMI / BMI2 one the host-pointer
 * paths use where the CPU has them (*simd_used says which ran).  Replaces the per-pattern copy of do_parallel_query's setup
 * (src/main/server.c:691-695). */
int femto_amd_host_pack_keys(const uint8_t* dense, int ndense, int bits, int64_t npats, const int32_t* plen, const uint16_t* flat,
                             const int64_t* starts, int force_scalar, uint64_t* keys_out, int* simd_used);
int femto_amd_get_rank_mode(const femto_amd_index_t* ix);

/* ---- profiling hooks ---------------------------------------------------------------------- */
/* Average duration (ms) of the launches of the named kernel ("count", "locate", "resolve", "regexp") since the last
 * reset, measured with HIP events on the stream the kernel was launched on; n_launches out. */
int femto_amd_kernel_time_ms(femto_amd_index_t* ix, const char* kernel, double* avg_ms, int64_t* n_launches);
void femto_amd_kernel_time_reset(femto_amd_index_t* ix);
void femto_amd_kernel_time_enable(femto_amd_index_t* ix, int on);

/* Compulsory HBM traffic of a batch (bench.py's roofline): runs the batch once with a line trace and reports how many
 * DISTINCT 128-byte lines of each derived array the count phase (count_lines[10]) and the row expansion + locate walk
 * (locate_lines[10]) loaded; *rows_out = rows located.  Regions: 0 packed lines (mode 3), 1 level table, 2 suffix
 * array / offsets of the marked rows, 3 / 4 level-1 / level-2 lines (mode 4), 5 text, 6 inverse suffix array, 7 rank
 * units, 8 per-character rank lines, 9 context table.
 * Device pointers as in femto_amd_count_device; blocking; not to be called while other calls use the handle. */
int femto_amd_trace_lines(femto_amd_index_t* ix, int64_t npats, const int32_t* d_plen, const uint16_t* d_pats,
                          const int64_t* d_starts, int max_occs_each, int64_t* count_lines, int64_t* locate_lines,
                          int64_t* rows_out);
/* ... and how many lines of each region the two phases of that LAST trace READ in all (the same line read for two patterns
 * counts twice): what an unsorted batch fetches when the structure is far larger than the caches. */
int femto_amd_trace_reads(const femto_amd_index_t* ix, int64_t* count_reads /* [10] */, int64_t* locate_reads /* [10] */);

/* ---- index construction (femto block-file writer) ------------------------- */
/* Builds a femto index directory (byte-identical to index_documents(map=NULL),
 * src/main/construct.c:572) from `ndocs` documents given as raw bytes.  The suffix array of the
 * prepared text (bytes+5, one SEOF per document; src/main/bwt_prepare.c:227-311, ordered as the
 * reference's test sorter orders it, src/main/bwt_qsufsort.c:176-240) is computed on the GPU.
 * params: "block_size=..,bucket_size=..,mark_period=.." (src/main/index.c:185-219) or NULL. */
int femto_amd_build_index(const char* out_dir, int ndocs, const uint8_t* const* docs, const int64_t* doc_lens,
                          const char* const* doc_infos, const char* params, int device);
/* Same, from a caller-supplied suffix array of the prepared text (host arrays); no GPU needed. */
int femto_amd_build_index_from_sa(const char* out_dir, int ndocs, const uint8_t* const* docs,
                                  const int64_t* doc_lens, const char* const* doc_infos,
                                  const char* params, const int64_t* sa);

/* flatten_index (src/main/index.c:2260; the femto_flatten tool): directory index -> one flattened file that
 * both femto and femto_amd_open read; byte-identical to the reference's output. */
int femto_amd_flatten_index(const char* index_dir, const char* out_path);

/* Test hook: encodes one binary sequence exactly as bseq_construct_forcetype does
 * (src/main/wtree.c:365; force_type -1 literal only, 0 automatic, 1 RLE only).  out may be NULL to size. */
int femto_amd_bseq_encode(const uint8_t* bits_msb_first, int64_t bitlen, int force_type, uint8_t* out,
                          int64_t cap, int64_t* out_len);

#ifdef __cplusplus
}
#endif
#endif
