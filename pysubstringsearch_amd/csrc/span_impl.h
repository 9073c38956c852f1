// span_impl.h -- match spans: for rows of (entry id, pattern), where in the entry the best match within the pattern's
// budget stands, how long it is and how close (include/pss.h, pss_reader_match_spans).
// Part of search.hip: included there behind edit_impl.h and line_index_impl.h, whose select_entries_kernel gives every
// row its entry; not a header for anybody else.  How one start position scores, and the key that orders the scores, is
// span_core.h -- plain C++ that tests/native/span_core.cpp runs start by start on the CPU.
//
// One wavefront per row.  A step hands the 64 lanes 64 consecutive start positions of the entry; every lane scores its own
// (span_start_key), the step's keys are reduced to their minimum over xor-shuffles, and the wave keeps the least key over
// the steps.  It stops after a step that found distance 0: the steps ascend, so nothing later can beat it.
// Everything that depends on the lane -- the `s < starts` branch and the loops inside the score -- closes before the
// shuffles; the trip counts are wave-wide (the steps come from the entry's length, the band's rows from L), and so is the
// early exit, which reads the reduced key.  Lane 0 writes the row's 12 bytes.
// Bounds: span_core.h states the reads of a score.  The kernel itself reads one byte at the entry's end (start + len <
// n: entry_bounds leaves it on the closing newline, or on the last byte of an unterminated last entry).

#include "span_core.h"

template <bool kFold, bool kEdits>
__global__ __launch_bounds__(256) void span_kernel(const ChunkDesc *chunks, const u32 *chunk_of, const u32 *start, const u32 *len,
                                                   const u32 *pat_of, const u8 *pbytes, const u64 *poff, const u8 *budget, const u8 *pvoid,
                                                   u64 rows, int32_t *out)
{
    const u32 lane = (u32)lane_id();
    const u64 waves = (u64)gridDim.x * (blockDim.x / kWave);
    for (u64 row = (u64)blockIdx.x * (blockDim.x / kWave) + (u32)wave_id(); row < rows; row += waves) {
        const ChunkDesc ch = chunks[chunk_of[row]];
        const u32 es = start[row], el = len[row], q = pat_of[row];
        const u32 elen = (ch.text[es + el] == '\n' ? es + el : ch.n) - es;      // the entry's TRUE length (line_len is short by one for an unterminated last entry)
        const u8 *pat = pbytes + poff[q];
        const u32 L = (u32)(poff[q + 1] - poff[q]), k = budget[q];
        const u32 starts = pvoid[q] ? 0u : span_starts(elen, L, kEdits);
        u64 best = kSpanNone;
        for (u32 base = 0; base < starts; base += kWave) {                     // (the same trips for every lane)
            const u32 s = base + lane;
            u64 key = kSpanNone;
            if (s < starts) key = span_start_key<kFold, kEdits>(ch.text, ch.n, es, elen, s, pat, L, k);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 other = __shfl_xor(key, o);
                key = other < key ? other : key;
            }
            best = key < best ? key : best;
            if ((best >> 35) == 0) break;                                      // (wave-wide: every lane holds the reduced key)
            if (starts - base <= (u32)kWave) break;                            // (no wrap of base at entries of nearly 2^32 bytes)
        }
        if (lane == 0) span_unkey(best, L, out + 3 * row);
    }
}

// rows (chunk, line) pairs the caller has validated, each with the index of its pattern; the patterns folded already where
// `fold`, kSpanPatPad zero bytes behind them.  One upload per array, two kernels, one download, ONE wait.
int match_spans_device(DeviceCtx *ctx, const ChunkDesc *d_chunks, const LineDesc *d_lines, const uint32_t *chunk_of, const uint32_t *line_of,
                       const uint32_t *pat_of, uint64_t rows, const uint8_t *pbytes, const uint64_t *poff, uint32_t nq, const uint8_t *budget,
                       const uint8_t *pvoid, bool edits, bool fold, int32_t *out)
{
    if (rows == 0) return PSS_OK;
    hipStream_t s = ctx->stream;
    const size_t ptotal = (size_t)poff[nq] + kSpanPatPad;
    const size_t off_bytes = ((size_t)nq + 1) * 8;
    PSS_TRY(ctx->slot[Q_LO].reserve(rows * 4));
    PSS_TRY(ctx->slot[Q_CNT].reserve(rows * 4));
    PSS_TRY(ctx->slot[Q_START].reserve(rows * 4));
    PSS_TRY(ctx->slot[Q_LEN].reserve(rows * 4));
    PSS_TRY(ctx->slot[Q_EIDX].reserve(rows * 4));
    PSS_TRY(ctx->slot[Q_BYTES].reserve(ptotal));
    PSS_TRY(ctx->slot[Q_OFF].reserve(off_bytes + 2 * (size_t)nq));
    PSS_TRY(ctx->slot[Q_OUT].reserve(rows * 12));
    u32 *d_chunk_of = ctx->slot[Q_LO].as<u32>(), *d_line_of = ctx->slot[Q_CNT].as<u32>();
    u32 *d_start = ctx->slot[Q_START].as<u32>(), *d_len = ctx->slot[Q_LEN].as<u32>(), *d_pat_of = ctx->slot[Q_EIDX].as<u32>();
    u8 *d_pbytes = ctx->slot[Q_BYTES].as<u8>();
    u64 *d_poff = ctx->slot[Q_OFF].as<u64>();
    u8 *d_budget = ctx->slot[Q_OFF].as<u8>() + off_bytes, *d_pvoid = d_budget + nq;
    int32_t *d_out = ctx->slot[Q_OUT].as<int32_t>();
    PSS_HIP(hipMemcpyAsync(d_chunk_of, chunk_of, rows * 4, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_line_of, line_of, rows * 4, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_pat_of, pat_of, rows * 4, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_pbytes, pbytes, ptotal, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_poff, poff, off_bytes, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_budget, budget, nq, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_pvoid, pvoid, nq, hipMemcpyHostToDevice, s));
    const u32 grid = (u32)std::min<u64>((u64)ctx->num_cus * 16, (rows + 255) / 256);
    hipLaunchKernelGGL(select_entries_kernel, dim3(grid), dim3(256), 0, s, d_chunks, d_lines, (const u32 *)d_chunk_of,
                       (const u32 *)d_line_of, rows, d_start, d_len);
    const u32 wgrid = (u32)std::min<u64>((u64)ctx->num_cus * 8, (rows + 3) / 4);       // a wave per row, 4 waves a workgroup
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(wgrid), dim3(256), 0, s, d_chunks, (const u32 *)d_chunk_of, (const u32 *)d_start, (const u32 *)d_len,
                           (const u32 *)d_pat_of, (const u8 *)d_pbytes, (const u64 *)d_poff, (const u8 *)d_budget, (const u8 *)d_pvoid, rows,
                           d_out);
    };
    if (fold) {
        if (edits) launch(span_kernel<true, true>); else launch(span_kernel<true, false>);
    } else {
        if (edits) launch(span_kernel<false, true>); else launch(span_kernel<false, false>);
    }
    PSS_HIP(hipGetLastError());
    PSS_HIP(hipMemcpyAsync(out, d_out, rows * 12, hipMemcpyDeviceToHost, s));
    PSS_HIP(hipStreamSynchronize(s));
    return PSS_OK;
}
