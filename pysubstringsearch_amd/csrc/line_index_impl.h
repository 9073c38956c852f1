// line_index_impl.h -- entry ids: the line index of a chunk (rank / select over its newlines), the emit kernel of the
// ids mode of the batch search, and the fetch of entry text by id.
// Part of search.hip: included there behind the entry helpers (zero_bytes, entry_bounds, copy_entry) and the workspace
// slots; not a header for anybody else.
//
// An entry id is (chunk index in the index file << 32) | line, line = the number of 0x0A bytes of the chunk's text
// before the entry's first byte.  The line index of a chunk is one u32 per block of B = 2^shift bytes of its text:
//   rank[j] = newlines in text[0, j * B),  j = 0 .. blocks  (rank[blocks] = all of them),
//   rank[blocks + 1] = entries of the chunk = rank[blocks] + (1 when the text does not end in a newline).
// rank (offset -> line): rank[start / B] + the newlines of text[(start / B) * B, start) -- one table read and B / 2
// bytes of text on average.  select (line -> offset): binary search for the block that holds the line-th newline, then
// a scan of that block.

struct InLenPlain {
    const u32 *len;
    __device__ u64 operator()(u64 i) const { return len[i]; }
};

__device__ __forceinline__ u32 newline_count16(const uint4 v)
{
    const u64 NL = 0x0a0a0a0a0a0a0a0aull;
    const u64 a = (u64)v.x | ((u64)v.y << 32), b = (u64)v.z | ((u64)v.w << 32);
    return (u32)__popcll(zero_bytes(a ^ NL)) + (u32)__popcll(zero_bytes(b ^ NL));
}

// Newlines per block.  A group of B / 16 lanes (4 .. 64: shift 6 .. 10) takes one block, one 16-byte load per lane --
// consecutive lanes read consecutive pieces, so a wave moves 1 KiB per instruction -- and adds up over xor-shuffles.
// Pieces that start at or behind n are not read (the text is readable 128 bytes past n, not a whole block); the
// piece that straddles n reads zero padding.
__global__ __launch_bounds__(256) void line_count_kernel(const u8 *text, u32 n, u32 shift, u32 blocks, u32 *cnt)
{
    const u32 gshift = shift - 4;
    const u64 pieces = (u64)blocks << gshift;
    const u64 bound = (pieces + kWave - 1) / kWave * kWave;          // whole waves: every lane takes part in the shuffles
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < bound; i += (u64)gridDim.x * blockDim.x) {
        u32 v = 0;
        if (i < pieces && i * 16 < n) v = newline_count16(reinterpret_cast<const uint4 *>(text)[i]);
        for (u32 o = 1; o < (1u << gshift); o <<= 1) v += __shfl_xor(v, (int)o);
        if (i < pieces && (i & ((1u << gshift) - 1)) == 0) cnt[i >> gshift] = v;
    }
}

// The scanned counts (u64, blocks + 1 of them) as the u32 table, and the chunk's entry count behind it.
__global__ __launch_bounds__(256) void line_rank_kernel(const u64 *scan, const u8 *text, u32 n, u32 blocks, u32 *rank)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= blocks; i += (u64)gridDim.x * blockDim.x) {
        rank[i] = (u32)scan[i];
        if (i == blocks) rank[blocks + 1] = (u32)scan[blocks] + ((n && text[n - 1] != '\n') ? 1u : 0u);
    }
}

int build_line_index(DeviceCtx *ctx, const uint8_t *d_text, uint32_t n, uint32_t shift, uint32_t *d_rank)
{
    if (shift < kLineShiftMin || shift > kLineShiftMax) {
        set_error("line index: block of 2^%u bytes (2^%u .. 2^%u)", shift, kLineShiftMin, kLineShiftMax);
        return PSS_EINVAL;
    }
    const u32 blocks = (u32)line_blocks(n, shift);
    PSS_TRY(ctx->slot[Q_SMALL].reserve(SC_MAX_BLOCKS * 8 + 256));
    PSS_TRY(ctx->slot[Q_LINE_TMP].reserve(((size_t)blocks + 1) * 8));
    u64 *partial = ctx->slot[Q_SMALL].as<u64>(), *d_total = partial + SC_MAX_BLOCKS;
    u64 *scan = ctx->slot[Q_LINE_TMP].as<u64>();
    const u64 pieces = (u64)blocks << (shift - 4);
    const u32 grid = (u32)std::min<u64>((pieces + 255) / 256, (u64)ctx->num_cus * 8);
    hipLaunchKernelGGL(line_count_kernel, dim3(grid ? grid : 1), dim3(256), 0, ctx->stream, d_text, n, shift, blocks, d_rank);
    PSS_TRY(device_excl_scan(ctx, InU32{d_rank}, (u64)blocks, partial, d_total, scan));
    const u32 grid2 = (u32)std::min<u64>(((u64)blocks + 256) / 256, (u64)ctx->num_cus * 8);
    hipLaunchKernelGGL(line_rank_kernel, dim3(grid2), dim3(256), 0, ctx->stream, (const u64 *)scan, d_text, n, blocks, d_rank);
    PSS_HIP(hipGetLastError());
    return PSS_OK;
}

// Newlines of text[from, to), from a multiple of 64 (a block start): 64 bytes per step as four 16-byte loads.  Reads up
// to 63 bytes past `to` (to < n: inside the zero padding).
__device__ __forceinline__ u32 newlines_between(const u8 *text, u32 from, u32 to)
{
    const u64 NL = 0x0a0a0a0a0a0a0a0aull;
    u32 c = 0;
    for (u32 p = from; p < to; p += 64) {
        const uint4 *q = reinterpret_cast<const uint4 *>(text + p);
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint4 x = v[k >> 1];
            const u64 w = (k & 1) ? ((u64)x.z | ((u64)x.w << 32)) : ((u64)x.x | ((u64)x.y << 32));
            u64 m = zero_bytes(w ^ NL);
            const u32 at = p + 8 * k;
            if (at >= to) m = 0;
            else if (to - at < 8) m &= (1ull << (8 * (to - at))) - 1ull;
            c += (u32)__popcll(m);
        }
    }
    return c;
}

// ids mode of the batch search: one id per kept hit at eidx[t], instead of emit_kernel's copy of the entry.  The
// "offsets" of the packed result are filled here as well (8 bytes per id).
__global__ __launch_bounds__(256) void emit_ids_kernel(const ChunkDesc *chunks, const LineDesc *lines, u32 nc, u64 nvq, const u64 *hit_off,
                                                         u64 H, const u32 *start, const u32 *len, const u64 *eidx, u64 *ent_off, u64 *ids)
{
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < H; t += (u64)gridDim.x * blockDim.x) {
        if (len[t] == kSkip) continue;
        const u32 c = (u32)(pair_of_hit(hit_off, nvq, t) % nc);
        const u8 *text = chunks[c].text;
        const LineDesc ld = lines[c];
        const u32 s = start[t], blk = s >> ld.shift;
        const u32 line = ld.rank[blk] + newlines_between(text, blk << ld.shift, s);
        const u64 e = eidx[t];
        ids[e] = ((u64)ld.file_index << 32) | line;
        ent_off[e] = 8 * e;
    }
}

// select: where entry `line` of chunk `c` starts, and how long it is.  The caller has checked line < entries, so the
// line-th newline exists and lies in the last block j with rank[j] < line (blocks without a newline repeat the rank of
// their successor: the search settles on the last of such a run, the one whose successor's rank reaches `line`).
__global__ __launch_bounds__(256) void select_entries_kernel(const ChunkDesc *chunks, const LineDesc *lines, const u32 *chunk_of,
                                                               const u32 *line_of, u64 n, u32 *start_out, u32 *len_out)
{
    const u64 NL = 0x0a0a0a0a0a0a0a0aull;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 c = chunk_of[i], line = line_of[i];
        const ChunkDesc ch = chunks[c];
        const LineDesc ld = lines[c];
        u32 s = 0;
        if (line) {
            u32 a = 0, b = ld.nblocks;               // rank[a] < line (rank[0] = 0), rank[b] >= line (or b = blocks)
            while (b - a > 1) {
                const u32 mid = a + (b - a) / 2;
                if (ld.rank[mid] < line) a = mid; else b = mid;
            }
            u32 need = line - ld.rank[a];            // the need-th newline of block a, counted from 1
            bool found = false;
            for (u32 p = a << ld.shift; !found && p < ch.n; p += 64) {
                const uint4 *q = reinterpret_cast<const uint4 *>(ch.text + p);
                uint4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = q[k];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const uint4 x = v[k >> 1];
                    const u64 w = (k & 1) ? ((u64)x.z | ((u64)x.w << 32)) : ((u64)x.x | ((u64)x.y << 32));
                    u64 m = zero_bytes(w ^ NL);
                    const u32 cnt = (u32)__popcll(m);
                    if (found) continue;
                    if (cnt < need) {
                        need -= cnt;
                        continue;
                    }
                    for (; need > 1; --need) m &= m - 1;
                    s = p + 8 * k + (u32)(__builtin_ctzll(m) >> 3) + 1;
                    found = true;
                }
            }
            if (!found || s >= ch.n) s = 0;          // (never for a line the chunk has)
        }
        u32 ls = 0, ll = 0;
        entry_bounds(ch, s, ls, ll);
        start_out[i] = ls;
        len_out[i] = ll;
    }
}

__global__ __launch_bounds__(256) void copy_entries_kernel(const ChunkDesc *chunks, const u32 *chunk_of, const u32 *start, const u32 *len,
                                                             const u64 *boff, u64 n, u8 *out)
{
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        copy_entry(out + boff[i], chunks[chunk_of[i]].text + start[i], len[i]);
}

int entries_by_id_device(DeviceCtx *ctx, const ChunkDesc *d_chunks, const LineDesc *d_lines, const uint32_t *chunk_of,
                         const uint32_t *line_of, uint64_t n, HostResult *res)
{
    hipStream_t s = ctx->stream;
    res->nq = n;
    res->n_entries = 0;
    res->n_bytes = 0;
    res->qcount = (u64 *)malloc((n ? n : 1) * sizeof(u64));
    if (!res->qcount) return PSS_ENOMEM;
    for (u64 i = 0; i < n; ++i) res->qcount[i] = 1;
    if (n == 0) {
        res->offsets = (u64 *)calloc(1, sizeof(u64));
        return res->offsets ? PSS_OK : PSS_ENOMEM;
    }
    PSS_TRY(ctx->slot[Q_LO].reserve(n * 4));
    PSS_TRY(ctx->slot[Q_CNT].reserve(n * 4));
    PSS_TRY(ctx->slot[Q_START].reserve(n * 4));
    PSS_TRY(ctx->slot[Q_LEN].reserve(n * 4));
    PSS_TRY(ctx->slot[Q_BOFF].reserve((n + 1) * 8));
    PSS_TRY(ctx->slot[Q_SMALL].reserve(SC_MAX_BLOCKS * 8 + 256));
    u32 *d_chunk_of = ctx->slot[Q_LO].as<u32>(), *d_line_of = ctx->slot[Q_CNT].as<u32>();
    u32 *d_start = ctx->slot[Q_START].as<u32>(), *d_len = ctx->slot[Q_LEN].as<u32>();
    u64 *d_boff = ctx->slot[Q_BOFF].as<u64>();
    u64 *d_partial = ctx->slot[Q_SMALL].as<u64>(), *d_total = d_partial + SC_MAX_BLOCKS;
    u64 *h_small = static_cast<u64 *>(ctx->pinned);
    PSS_HIP(hipMemcpyAsync(d_chunk_of, chunk_of, n * 4, hipMemcpyHostToDevice, s));
    PSS_HIP(hipMemcpyAsync(d_line_of, line_of, n * 4, hipMemcpyHostToDevice, s));
    const u32 grid = (u32)std::min<u64>((u64)ctx->num_cus * 16, (n + 255) / 256);
    hipLaunchKernelGGL(select_entries_kernel, dim3(grid), dim3(256), 0, s, d_chunks, d_lines, (const u32 *)d_chunk_of,
                       (const u32 *)d_line_of, n, d_start, d_len);
    PSS_TRY(device_excl_scan(ctx, InLenPlain{d_len}, n, d_partial, d_total, d_boff));
    PSS_HIP(hipMemcpyAsync(h_small, d_total, 8, hipMemcpyDeviceToHost, s));
    PSS_HIP(hipStreamSynchronize(s));
    const u64 B = h_small[0];
    PSS_TRY(ctx->slot[Q_OUT].reserve(B + 16));
    u8 *d_out = ctx->slot[Q_OUT].as<u8>();
    hipLaunchKernelGGL(copy_entries_kernel, dim3(grid), dim3(256), 0, s, d_chunks, (const u32 *)d_chunk_of, (const u32 *)d_start,
                       (const u32 *)d_len, (const u64 *)d_boff, n, d_out);
    PSS_TRY(alloc_host_result(res, n, B, !search_knobs().no_pinned_results));
    PSS_HIP(hipMemcpyAsync(res->offsets, d_boff, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    if (B) PSS_HIP(hipMemcpyAsync(res->bytes, d_out, B, hipMemcpyDeviceToHost, s));
    PSS_HIP(hipStreamSynchronize(s));
    PSS_HIP(hipGetLastError());
    res->n_entries = n;
    res->n_bytes = B;
    return PSS_OK;
}
