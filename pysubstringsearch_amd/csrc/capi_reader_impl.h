// The Reader side of the C ABI: opening an index (one GPU, a shard of it, or several GPUs in one process), the residency manager, the batch / count / device-result calls and the merge of packed results.
// Part of capi.cpp: included there, in this order, into the one translation unit (the pieces share its
// anonymous-namespace helpers); not a header for anybody else.

// ------------------------------------------------------------------- Reader --

struct pss_reader {
    int device = 0;
    DeviceCtx *ctx = nullptr;
    std::vector<ChunkDesc> chunks;      // device pointers of resident chunks
    // Residency of chunk i.  The text always lives in HBM.  The suffix array does too while it fits;
    // past the HBM budget it stays in pinned host memory that the kernels read over PCIe (tier 2:
    // the key-sample table, kept in HBM, confines every query to a few dozen such reads).
    struct Mem {
        void *text = nullptr;
        void *sa = nullptr;        // hipMalloc or (sa_host) hipHostMalloc
        void *skeys = nullptr;     // own hipMalloc when the suffix array is on the host, else inside `sa`
        bool sa_host = false;
        uint64_t hbm_bytes = 0, host_bytes = 0;
        // Line index behind the entry ids (search.h, LineDesc): built by the first call that asks for ids, always in HBM,
        // counted in hbm_bytes from then on, never moved by the residency manager.
        void *lines = nullptr;
        uint64_t lines_bytes = 0;
        uint32_t line_shift = 0, entries = 0;
        bool lines_built = false;
    };
    std::vector<Mem> mem;
    std::vector<uint64_t> file_index;   // chunk i's index in the index file (a shard holds every k-th): the high word of its entry ids
    LineDesc *d_lines = nullptr;        // device copy of the line tables' descriptors, parallel to d_descs
    size_t d_lines_cap = 0;
    ChunkDesc *d_descs = nullptr;
    size_t d_descs_cap = 0;
    bool dirty = true;
    bool low_latency = false;            // single queries through the resident kernel (pss_reader_set_low_latency)
    // entries of one chunk in the reference's order (suffix-array order of their first hit, src/lib.rs:262-276) instead of
    // the order of their leftmost match: pss_reader_set_result_order, PSS_RESULT_ORDER=sa
    bool order_sa = knob("PSS_RESULT_ORDER") != nullptr && strcmp(knob("PSS_RESULT_ORDER"), "sa") == 0;
    // Residency manager ("LRU when index > HBM").  A reader with suffix arrays on the host tier keeps,
    // per chunk, a decayed count of the hits its batches found there and the number of the last batch that touched it;
    // between batches the hottest host-tier suffix array changes places with the coldest one in HBM when it is more than
    // twice as hot (one exchange per batch; PSS_READER_AUTO_RESIDENCY=0: never -- evict / promote stay as overrides).
    std::vector<uint64_t> heat, last_touch, batch_hits;
    std::vector<uint8_t> manual;         // chunks the caller placed by hand (evict / promote): the manager leaves them alone
    uint64_t batch_seq = 0, auto_moves = 0;
    bool auto_residency = knob("PSS_READER_AUTO_RESIDENCY") == nullptr || atoi(knob("PSS_READER_AUTO_RESIDENCY")) != 0;
    pss_search_stats last{};
    // A reader over several devices (pss_reader_open_multi) is a front for one reader per device -- part k holds the
    // chunks c with c % G == k on devices[k] -- each with a worker thread that answers the batch for its chunks; the
    // calling thread takes part 0 itself and merges (reference: rayon fans one search over all chunks inside the
    // process, src/lib.rs:207, 280-284).
    struct Part;
    std::vector<Part *> parts;
    std::mutex multi_mu;                 // one batch at a time through the workers
};

struct pss_reader::Part {
    pss_reader *reader = nullptr;        // plain single-device reader of this part's chunks
    std::thread worker;
    std::mutex mu;
    std::condition_variable cv;
    // mailbox: the caller fills the job and raises `pending`; the worker clears it when `rc` / `res` / `err` are set
    bool pending = false, quit = false;
    SearchRequest rq;                    // SEARCH_FULL / SEARCH_COUNTS / SEARCH_IDS; plain, anchored or all-terms
    int rc = 0;
    HostResult res;
    std::string err;
};

struct pss_result {
    HostResult r;
};

namespace {

int reader_sync_descs(pss_reader *r);
int reader_ensure_lines(pss_reader *r);

// HBM the reader may still take for suffix arrays: PSS_READER_HBM_BUDGET (bytes, over all chunks of
// this reader; tests use it to force the host tier), else whatever hipMalloc grants while
// kHbmReserve stays free for the search and build workspaces.
constexpr size_t kHbmReserve = (size_t)2 << 30;

void reader_free_mem(pss_reader::Mem &m)
{
    if (m.text) (void)hipFree(m.text);
    if (m.sa) (void)(m.sa_host ? hipHostFree(m.sa) : hipFree(m.sa));
    if (m.skeys) (void)hipFree(m.skeys);
    if (m.lines) (void)hipFree(m.lines);
    m = pss_reader::Mem{};
}

void reader_drop_lines(pss_reader::Mem &m)
{
    if (m.lines) (void)hipFree(m.lines);
    m.hbm_bytes -= m.lines_bytes;
    m.lines = nullptr;
    m.lines_bytes = 0;
    m.entries = 0;
    m.lines_built = false;
}

// Text (zero padded) and suffix array of one chunk; the key-sample table (search.h) lives behind
// the suffix array in the same allocation (or on its own in HBM when the suffix array is on the host).
uint64_t *reader_hits_buffer(pss_reader *r);
void reader_note_batch(pss_reader *r);

int reader_alloc_chunk(pss_reader *r, uint32_t n, ChunkDesc *out, pss_reader::Mem *mem)
{
    PSS_HIP(hipSetDevice(r->device));
    pss_reader::Mem m;
    const size_t sa_bytes = round_up((size_t)n * 4 + 16, 8);
    const bool samples = knob("PSS_NO_KEY_SAMPLES") == nullptr;
    uint32_t shift = kSampleShift;
    if (const char *ev = knob("PSS_SAMPLE_SHIFT")) {      // tests: dense tables on small chunks
        const int v = atoi(ev);
        if (v >= 0 && v <= 20) shift = (uint32_t)v;
    }
    const size_t sk_bytes = samples ? sample_count(n, shift) * 8 : 0;
    hipError_t e = hipMalloc(&m.text, (size_t)n + 128);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("hipMalloc of the text of a %u-byte chunk failed: %s", n, hipGetErrorString(e));
        return PSS_ENOMEM;
    }
    m.hbm_bytes = (size_t)n + 128;
    // tier 1: suffix array (+ samples) in HBM
    uint64_t used = 0;
    for (const auto &x : r->mem) used += x.hbm_bytes;
    bool want_hbm = true;
    if (const char *ev = knob("PSS_READER_HBM_BUDGET"))
        want_hbm = used + m.hbm_bytes + sa_bytes + sk_bytes <= strtoull(ev, nullptr, 0);
    // (second attempt: the grow-only workspace of the builder on this device -- up to 80 bytes per byte of the largest
    // chunk it has built, the sample sort's element buffers alone 32 -- goes back before a suffix array settles for the
    // host tier; the next build allocates what it needs again)
    for (int attempt = 0; want_hbm && attempt < 2 && !m.sa; ++attempt) {
        if (attempt == 1) {
            {
                std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
                r->ctx->stop_resident();
                for (auto &sl : r->ctx->slot) sl.release();
                r->ctx->small_hdr_ready = nullptr;
            }
            DeviceCtx *bctx = nullptr;                 // (lock order: reader side, then builder side -- nothing takes them the other way round)
            if (get_build_ctx(r->device, &bctx) == PSS_OK) {
                std::lock_guard<std::recursive_mutex> lk(bctx->mu);
                for (auto &sl : bctx->slot) sl.release();
                if (bctx->helper)
                    for (auto &sl : bctx->helper->slot) sl.release();
            }
        }
        e = hipMalloc(&m.sa, sa_bytes + sk_bytes);
        if (e == hipSuccess) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < kHbmReserve && !knob("PSS_READER_HBM_BUDGET")) {
                (void)hipFree(m.sa);                  // it fits, but would starve the workspaces
                m.sa = nullptr;
            }
        } else {
            (void)hipGetLastError();
            m.sa = nullptr;
        }
    }
    if (m.sa) {
        m.hbm_bytes += sa_bytes + sk_bytes;
        out->skeys = samples ? reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(m.sa) + sa_bytes) : nullptr;
    } else {
        // tier 2: suffix array in pinned host memory, samples in HBM
        e = hipHostMalloc(&m.sa, sa_bytes, hipHostMallocPortable);
        if (e == hipSuccess && sk_bytes) e = hipMalloc(&m.skeys, sk_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            m.sa_host = m.sa != nullptr;
            reader_free_mem(m);
            set_error("no room for the suffix array of a %u-byte chunk in HBM or pinned host memory: %s", n,
                      hipGetErrorString(e));
            return PSS_ENOMEM;
        }
        m.sa_host = true;
        m.host_bytes = sa_bytes;
        m.hbm_bytes += sk_bytes;
        out->skeys = static_cast<uint64_t *>(m.skeys);
    }
    PSS_HIP(hipMemsetAsync(static_cast<uint8_t *>(m.text) + n, 0, 128, r->ctx->stream));
    out->text = static_cast<uint8_t *>(m.text);
    if (m.sa_host) {
        void *dp = nullptr;
        PSS_HIP(hipHostGetDevicePointer(&dp, m.sa, 0));
        out->sa = static_cast<uint32_t *>(dp);
    } else {
        out->sa = static_cast<uint32_t *>(m.sa);
    }
    out->n = n;
    out->shift = shift;
    *mem = m;
    return PSS_OK;
}

// (Re)builds the key samples of a chunk whose text and suffix array are in place (stream-ordered).
int reader_sample_chunk(pss_reader *r, const ChunkDesc &c)
{
    if (!c.skeys) return PSS_OK;
    return build_key_samples(r->ctx, c.text, c.sa, c.n, c.shift, const_cast<uint64_t *>(c.skeys));
}

void reader_free(pss_reader *r);

// PSS_ROUTE_KEY_SAMPLES of the last batch: whether the chunks have key-sample tables was decided when they were loaded
// (reader_alloc_chunk), not by search_batch_device, which sees the chunk table only on the device.
void reader_note_route(pss_reader *r)
{
    for (const ChunkDesc &c : r->chunks)
        if (c.skeys) {
            r->last.route |= PSS_ROUTE_KEY_SAMPLES;
            return;
        }
}

int multi_batch(pss_reader *r, const SearchRequest &rq, HostResult *out);

// One batch on whatever kind of reader r is: the one way from every entry point below to search_batch_device.  The caller
// states queries, mode and anchors; the reader's settings supply the rest.
int reader_batch(pss_reader *r, SearchRequest rq, HostResult *res)
{
    if (!r->parts.empty()) return multi_batch(r, rq, res);
    std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
    PSS_HIP(hipSetDevice(r->device));
    PSS_TRY(reader_sync_descs(r));
    if (rq.mode == SEARCH_IDS) PSS_TRY(reader_ensure_lines(r));
    rq.sa_order = r->order_sa;
    rq.low_latency = r->low_latency && rq.mode == SEARCH_FULL && !rq.anchors && !rq.group_offsets;
    rq.chunk_hits = rq.mode == SEARCH_DEVICE ? nullptr : reader_hits_buffer(r);     // (device results have never fed the residency manager)
    PSS_TRY(search_batch_device(r->ctx, r->d_descs, r->d_lines, (uint32_t)r->chunks.size(), rq, res, &r->last));
    reader_note_route(r);
    if (rq.chunk_hits) reader_note_batch(r);
    return PSS_OK;
}

void part_run(pss_reader::Part *p)      // the job in p's mailbox, on p's reader
{
    p->res.release();
    p->err.clear();
    p->rc = reader_batch(p->reader, p->rq, &p->res);
    if (p->rc != PSS_OK) p->err = last_error();
}

void part_worker(pss_reader::Part *p)
{
    std::unique_lock<std::mutex> lk(p->mu);
    for (;;) {
        p->cv.wait(lk, [&] { return p->pending || p->quit; });
        if (p->quit) return;
        part_run(p);
        p->pending = false;
        p->cv.notify_all();
    }
}

void reader_free(pss_reader *r)
{
    if (!r) return;
    for (pss_reader::Part *p : r->parts) {
        if (p->worker.joinable()) {
            {
                std::lock_guard<std::mutex> lk(p->mu);
                p->quit = true;
            }
            p->cv.notify_all();
            p->worker.join();
        }
        p->res.release();
        reader_free(p->reader);
        delete p;
    }
    r->parts.clear();
    if (r->ctx) (void)hipSetDevice(r->device);
    if (r->ctx) {
        std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
        if (r->ctx->resident.running && r->ctx->resident.chunks == r->d_descs) r->ctx->stop_resident();   // it reads r's chunk table
    }
    for (auto &m : r->mem) reader_free_mem(m);
    if (r->d_descs) (void)hipFree(r->d_descs);
    if (r->d_lines) (void)hipFree(r->d_lines);
    delete r;
}

// Reads `bytes` from fp's current position into host memory with the I/O pool (pieces of 16 MiB, several threads).
// (stripes: the bytes are units unit_base, unit_base + 1, .. of the striped layout's files instead of fp's next bytes)
int read_file_parallel(FILE *fp, void *dst, size_t bytes, const Stripes *stripes = nullptr, uint64_t unit_base = 0)
{
    const int fd = fileno(fp);
    const int64_t base = (int64_t)ftello(fp);
    const size_t piece = DeviceCtx::kIoPiece;
    IoPool::Batch batch;
    for (size_t o = 0; o < bytes; o += piece) {
        if (stripes) {
            const uint64_t u = unit_base + o / piece;
            const uint64_t S = (uint64_t)stripes->S();
            IoPool::get().submit(&batch, stripes->fd[(size_t)(u % S)], false, static_cast<uint8_t *>(dst) + o, std::min(piece, bytes - o),
                                 (int64_t)((u / S) * piece));
        } else
            IoPool::get().submit(&batch, fd, false, static_cast<uint8_t *>(dst) + o, std::min(piece, bytes - o), base + (int64_t)o);
    }
    const int err = IoPool::wait_all(&batch);
    if (err) {
        set_error("failed to fill whole buffer (truncated index file)");   // UnexpectedEof
        return PSS_EFORMAT;
    }
    if (!stripes && fseeko(fp, (off_t)(base + (int64_t)bytes), SEEK_SET) != 0) return io_error("seek");
    return PSS_OK;
}

// Reads `bytes` from fp's current position into device memory: the threads of the I/O pool pread pieces into a ring of
// pinned buffers (up to kIoPieces reads in flight), the copy stream uploads every piece as soon as it has arrived --
// reading, uploading and the page-cache copies of several pieces overlap (round 3: one thread's fread, then the copy).
int upload_from_file(pss_reader *r, FILE *fp, void *dst, size_t bytes, const Stripes *stripes = nullptr, uint64_t unit_base = 0)
{
    DeviceCtx *ctx = r->ctx;
    PSS_TRY(ctx->ensure_io_ring());
    const int fd = fileno(fp);
    const int64_t base = (int64_t)ftello(fp);
    const size_t piece = DeviceCtx::kIoPiece;
    constexpr int S = DeviceCtx::kIoPieces;
    const size_t pieces = (bytes + piece - 1) / piece;
    IoPool::Batch batch;
    IoPool &pool = IoPool::get();
    std::atomic<int> done[S];
    for (auto &x : done) x.store(1);
    size_t next = 0;
    bool short_read = false;
    auto body = [&]() -> int {
        for (size_t i = 0; i < pieces; ++i) {
            while (next < pieces && next < i + (size_t)S) {
                const int slot = (int)(next % S);
                if (next >= (size_t)S) PSS_HIP(hipEventSynchronize(ctx->io_ev[slot]));   // the upload of piece next - S is through
                const size_t o = next * piece;
                if (stripes) {
                    const uint64_t u = unit_base + next, SS = (uint64_t)stripes->S();
                    pool.submit(&batch, stripes->fd[(size_t)(u % SS)], false, ctx->io_ring[slot], std::min(piece, bytes - o),
                                (int64_t)((u / SS) * piece), &done[slot]);
                } else
                    pool.submit(&batch, fd, false, ctx->io_ring[slot], std::min(piece, bytes - o), base + (int64_t)o, &done[slot]);
                ++next;
            }
            const int slot = (int)(i % S);
            IoPool::wait_flag(&batch, &done[slot]);
            {
                std::lock_guard<std::mutex> lk(batch.mu);
                if (batch.err) { short_read = true; return PSS_OK; }
            }
            const size_t o = i * piece, k = std::min(piece, bytes - o);
            PSS_HIP(hipMemcpyAsync(static_cast<uint8_t *>(dst) + o, ctx->io_ring[slot], k, hipMemcpyHostToDevice, ctx->copy_stream));
            PSS_HIP(hipEventRecord(ctx->io_ev[slot], ctx->copy_stream));
        }
        return PSS_OK;
    };
    const int rc = body();
    const int err = IoPool::wait_all(&batch);          // always: the pool's pieces point at `done` and at the ring
    const hipError_t he = hipStreamSynchronize(ctx->copy_stream);
    if (rc != PSS_OK) return rc;
    if (err || short_read) {
        set_error("failed to fill whole buffer (truncated index file)");   // UnexpectedEof
        return PSS_EFORMAT;
    }
    PSS_HIP(he);
    if (!stripes && fseeko(fp, (off_t)(base + (int64_t)bytes), SEEK_SET) != 0) return io_error("seek");
    return PSS_OK;
}

}  // namespace

namespace {
// Device copy of the chunk descriptor array (re-uploaded whenever chunks change).
int reader_sync_descs(pss_reader *r)
{
    const uint32_t nc = (uint32_t)r->chunks.size();
    if (!r->dirty || nc == 0) return PSS_OK;
    r->ctx->stop_resident();             // (a resident search kernel keeps reading the table it was started with)
    if (r->d_descs_cap < nc) {
        if (r->d_descs) (void)hipFree(r->d_descs);
        r->d_descs = nullptr;
        const size_t cap = nc < 16 ? 16 : (size_t)nc * 2;
        PSS_HIP(hipMalloc(reinterpret_cast<void **>(&r->d_descs), sizeof(ChunkDesc) * cap));
        r->d_descs_cap = cap;
    }
    PSS_HIP(hipMemcpy(r->d_descs, r->chunks.data(), sizeof(ChunkDesc) * nc, hipMemcpyHostToDevice));
    r->dirty = false;
    return PSS_OK;
}

// The line index of every resident chunk that has none yet -- all of them on the first call that asks for ids, later the
// chunks pss_reader_add_chunk_device appended or pss_reader_set_chunk_device replaced -- and the device copy of the
// descriptors.  A reader that never asks for ids never gets here.  (The caller holds the context and has made the
// device current.)
int reader_ensure_lines(pss_reader *r)
{
    const size_t nc = r->chunks.size();
    uint32_t shift = kLineShift;
    if (const char *ev = knob("PSS_LINE_BLOCK_SHIFT")) {
        const int v = atoi(ev);
        if (v >= (int)kLineShiftMin && v <= (int)kLineShiftMax) shift = (uint32_t)v;
    }
    std::vector<size_t> fresh;
    for (size_t c = 0; c < nc; ++c) {
        pss_reader::Mem &m = r->mem[c];
        const ChunkDesc &cd = r->chunks[c];
        if (m.lines_built || cd.n == 0) continue;
        if (!m.lines) {
            const size_t bytes = line_table_bytes(cd.n, shift);
            const hipError_t e = hipMalloc(&m.lines, bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                m.lines = nullptr;
                set_error("hipMalloc of the line index of a %u-byte chunk failed: %s", cd.n, hipGetErrorString(e));
                return PSS_ENOMEM;
            }
            m.lines_bytes = bytes;
            m.hbm_bytes += bytes;
            m.line_shift = shift;
        }
        PSS_TRY(build_line_index(r->ctx, cd.text, cd.n, m.line_shift, static_cast<uint32_t *>(m.lines)));
        fresh.push_back(c);
    }
    if (fresh.empty() && r->d_lines) return PSS_OK;
    PSS_HIP(hipStreamSynchronize(r->ctx->stream));
    for (size_t c : fresh) {
        pss_reader::Mem &m = r->mem[c];
        const uint32_t *rank = static_cast<const uint32_t *>(m.lines);
        PSS_HIP(hipMemcpy(&m.entries, rank + line_blocks(r->chunks[c].n, m.line_shift) + 1, 4, hipMemcpyDeviceToHost));
        m.lines_built = true;
    }
    if (nc == 0) return PSS_OK;
    if (r->d_lines_cap < nc) {
        if (r->d_lines) (void)hipFree(r->d_lines);
        r->d_lines = nullptr;
        r->d_lines_cap = 0;
        const size_t cap = nc < 16 ? 16 : nc * 2;
        PSS_HIP(hipMalloc(reinterpret_cast<void **>(&r->d_lines), sizeof(LineDesc) * cap));
        r->d_lines_cap = cap;
    }
    std::vector<LineDesc> ld(nc);
    for (size_t c = 0; c < nc; ++c) {
        const pss_reader::Mem &m = r->mem[c];
        ld[c] = LineDesc{static_cast<const uint32_t *>(m.lines), m.lines_built ? (uint32_t)line_blocks(r->chunks[c].n, m.line_shift) : 0u,
                         m.line_shift, m.entries, (uint32_t)r->file_index[c]};
    }
    PSS_HIP(hipMemcpy(r->d_lines, ld.data(), sizeof(LineDesc) * nc, hipMemcpyHostToDevice));
    return PSS_OK;
}
}  // namespace

extern "C" int pss_reader_create(int32_t device, pss_reader **out)
{
    return guarded([&]() -> int {
        if (!out) return PSS_EINVAL;
        DeviceCtx *ctx;
        PSS_TRY(get_ctx(device, &ctx));
        pss_reader *r = new pss_reader();
        r->device = device;
        r->ctx = ctx;
        *out = r;
        return PSS_OK;
    });
}

extern "C" int pss_reader_open(const char *path, int32_t device, int32_t shard_index, int32_t shard_count,
                               pss_reader **out)
{
    return guarded([&]() -> int {
        if (!path || !out || shard_count < 1 || shard_index < 0 || shard_index >= shard_count) {
            set_error("pss_reader_open: bad arguments");
            return PSS_EINVAL;
        }
        if (device == -1) {             // the default list (PSS_DEVICES / a launcher's pin / every visible device)
            int32_t defaults[64];
            const int32_t k = pss_default_devices(defaults, 64);
            if (k < 1) return PSS_EINVAL;               // (a PSS_DEVICES that does not parse: the message is set)
            if (k > 1 && shard_count == 1) return pss_reader_open_multi(path, defaults, k, out);
            device = defaults[0];       // (a shard is one process's share: one device)
        }
        errno = 0;
        FILE *fp = fopen(path, "rb");   // File::open, lib.rs:165 (NotFound -> FileNotFoundError)
        if (!fp) return io_error(path);
        struct Closer {
            FILE *f;
            ~Closer() { fclose(f); }
        } closer{fp};
        if (fseeko(fp, 0, SEEK_END) != 0) return io_error(path);
        const uint64_t flen = (uint64_t)ftello(fp);   // fs::metadata().len(), lib.rs:168-169
        fseeko(fp, 0, SEEK_SET);
        DeviceCtx *ctx;
        PSS_TRY(get_ctx(device, &ctx));
        // The device context (staging buffers, streams) is shared with every other handle on the device: it is
        // held chunk by chunk, around the uploads only, so searches of other readers and Writer builds
        // interleave with a long load instead of waiting for the whole file.
        std::unique_lock<std::recursive_mutex> lk(ctx->mu, std::defer_lock);
        pss_reader *r = new pss_reader();
        r->device = device;
        r->ctx = ctx;
        uint64_t bytes_read = 0;
        int64_t index = 0;
        int rc = PSS_OK;
        // format 2 announces itself (a reference file starts with the u32 length of its first chunk,
        // < 2^30, which these bytes are not): 64-bit lengths, otherwise the same records
        bool v2 = false;
        Stripes stripes;                       // striped layout: the suffix arrays' files
        struct CloseStripes {
            Stripes &s;
            ~CloseStripes() { s.close_all(); }
        } close_stripes{stripes};
        if (flen >= kHeaderV2) {
            uint8_t fh[kHeaderV2];
            if (fread(fh, 1, kHeaderV2, fp) == kHeaderV2 && memcmp(fh, kMagicV2, 8) == 0) {
                v2 = true;
                bytes_read = kHeaderV2;
                const uint32_t fl = (uint32_t)fh[8] | ((uint32_t)fh[9] << 8) | ((uint32_t)fh[10] << 16) | ((uint32_t)fh[11] << 24);
                if (fl & kStripedFlag) {
                    const int S = (int)((fl >> 8) & 0xffu), ul = (int)((fl >> 16) & 0xffu);
                    if (S < 1 || S > 64 || ul != kStripeUnitLog || (fl & ~0x00ffff01u)) {
                        set_error("striped index: unknown header flags %#x", fl);
                        return PSS_EFORMAT;
                    }
                    for (int j = 0; j < S; ++j) {
                        errno = 0;
                        const int sf = open(Stripes::name(path, j).c_str(), O_RDONLY | O_CLOEXEC);
                        if (sf < 0) return io_error(Stripes::name(path, j).c_str());
                        stripes.fd.push_back(sf);
                    }
                } else if (fl) {
                    set_error("index file: unknown header flags %#x", fl);
                    return PSS_EFORMAT;
                }
            } else {
                fseeko(fp, 0, SEEK_SET);
            }
        }
        const bool striped = stripes.S() != 0;
        const size_t hl = v2 ? 8 : 4;
        auto get_len = [&](uint64_t *out_len) -> bool {
            uint8_t hdr[8];
            if (fread(hdr, 1, hl, fp) != hl) return false;
            uint64_t v = 0;
            for (size_t i = 0; i < hl; ++i) v |= (uint64_t)hdr[i] << (8 * i);
            *out_len = v;
            return true;
        };
        const char *kTrunc = "failed to fill whole buffer (truncated index file)";
        while (bytes_read < flen) {   // lib.rs:174
            if (lk.owns_lock()) lk.unlock();
            uint64_t dlen64 = 0, slen = 0;
            if (!get_len(&dlen64)) { set_error("%s", kTrunc); rc = PSS_EFORMAT; break; }
            if (dlen64 > (uint64_t)INT32_MAX || bytes_read + 2 * hl + dlen64 > flen) {
                if (dlen64 > (uint64_t)INT32_MAX && bytes_read + 2 * hl + dlen64 <= flen)
                    set_error("chunk %lld: %llu bytes of text exceed the 32-bit suffix array", (long long)index, (unsigned long long)dlen64);
                else
                    set_error("%s", kTrunc);
                rc = PSS_EFORMAT;
                break;
            }
            const uint32_t dlen = (uint32_t)dlen64;
            const bool mine = (index % shard_count) == shard_index;
            ChunkDesc cd{};
            pss_reader::Mem cm;
            if (mine && dlen) {
                lk.lock();
                rc = reader_alloc_chunk(r, dlen, &cd, &cm);
                if (rc) break;
                r->chunks.push_back(cd);
                r->mem.push_back(cm);
                r->file_index.push_back((uint64_t)index);
                rc = upload_from_file(r, fp, const_cast<uint8_t *>(cd.text), dlen);
                if (rc) break;
            } else if (fseeko(fp, dlen, SEEK_CUR) != 0) { rc = io_error(path); break; }
            if (!get_len(&slen)) { set_error("%s", kTrunc); rc = PSS_EFORMAT; break; }
            // the reference format stores (4n) as u32, which wraps from 2^30 bytes of text on (lib.rs:116)
            const uint64_t want = v2 ? (uint64_t)dlen * 4 : (uint64_t)(uint32_t)((uint64_t)dlen * 4);
            if (slen != want) {
                set_error("chunk %lld: suffix array of %llu bytes does not match %u bytes of text", (long long)index,
                          (unsigned long long)slen, dlen);
                rc = PSS_EFORMAT;
                break;
            }
            const uint64_t sa_bytes_all = (uint64_t)dlen * 4;
            const uint64_t sa_bytes_file = striped ? 0 : sa_bytes_all;        // (striped: the array is not in this file)
            if (bytes_read + 2 * hl + dlen + sa_bytes_file > flen) { set_error("%s", kTrunc); rc = PSS_EFORMAT; break; }
            const uint64_t unit_base = stripes.next_unit;
            if (striped) stripes.next_unit += (sa_bytes_all + DeviceCtx::kIoPiece - 1) / DeviceCtx::kIoPiece;
            if (mine && dlen) {
                if (cm.sa_host) {      // host tier: the file is read straight into the pinned buffer
                    rc = read_file_parallel(fp, cm.sa, (size_t)sa_bytes_all, striped ? &stripes : nullptr, unit_base);
                } else {
                    rc = upload_from_file(r, fp, cm.sa, (size_t)sa_bytes_all, striped ? &stripes : nullptr, unit_base);
                }
                if (rc) break;
                rc = reader_sample_chunk(r, cd);     // uploads are complete (copy stream synchronised)
                if (rc) break;
            } else if (sa_bytes_file && fseeko(fp, (off_t)sa_bytes_file, SEEK_CUR) != 0) { rc = io_error(path); break; }
            bytes_read += 2 * hl + (uint64_t)dlen + sa_bytes_file;   // lib.rs:184
            ++index;
        }
        if (!lk.owns_lock()) lk.lock();
        if (rc == PSS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) {
            set_error("key samples: %s", hipGetErrorString(hipGetLastError()));
            rc = PSS_EDEVICE;
        }
        if (rc == PSS_OK) rc = reader_sync_descs(r);
        if (rc != PSS_OK) {
            reader_free(r);
            return rc;
        }
        *out = r;
        return PSS_OK;
    });
}

extern "C" int pss_reader_open_multi(const char *path, const int32_t *devices, int32_t n_devices, pss_reader **out)
{
    return guarded([&]() -> int {
        if (!path || !out || !devices || n_devices < 1 || n_devices > 64) {
            set_error("pss_reader_open_multi: bad arguments");
            return PSS_EINVAL;
        }
        if (n_devices == 1) return pss_reader_open(path, devices[0], 0, 1, out);
        // every part reads the file for its own chunks (seeking over the others'), all parts at once: the uploads of
        // different devices overlap, parts sharing a device take turns on its staging buffers
        const int G = n_devices;
        std::vector<pss_reader *> rd(G, nullptr);
        std::vector<int> rcs(G, PSS_OK);
        std::vector<std::string> errs(G);
        std::vector<int> errnos(G, 0);
        std::vector<std::thread> th;
        for (int k = 0; k < G; ++k)
            th.emplace_back([&, k] {
                rcs[k] = pss_reader_open(path, devices[k], k, G, &rd[k]);
                if (rcs[k] != PSS_OK) {
                    errs[k] = last_error();
                    errnos[k] = errno;
                }
            });
        for (auto &t : th) t.join();
        for (int k = 0; k < G; ++k) {
            if (rcs[k] == PSS_OK) continue;
            set_error("%s", errs[k].c_str());
            const int rc = rcs[k], en = errnos[k];
            for (pss_reader *x : rd) reader_free(x);
            errno = en;       // (PSS_EIO: the binding turns errno into the OSError subclass the reference raises)
            return rc;
        }
        pss_reader *r = new pss_reader();
        r->device = devices[0];
        r->ctx = rd[0]->ctx;
        for (int k = 0; k < G; ++k) {
            pss_reader::Part *p = new pss_reader::Part();
            p->reader = rd[k];
            r->parts.push_back(p);
        }
        for (int k = 1; k < G; ++k) r->parts[k]->worker = std::thread(part_worker, r->parts[k]);      // part 0 runs on the caller
        *out = r;
        return PSS_OK;
    });
}

namespace {

// One batch over the parts of a multi-device reader: every worker answers for its chunks, the caller for part 0;
// then the per-part results are merged query-major, part-major inside a query (pss_merge_packed's order).  The "queries"
// of the merge are the rows of the results: the groups of an all-terms batch.
int multi_batch(pss_reader *r, const SearchRequest &rq, HostResult *out)
{
    const uint32_t nq = rq.rows();
    std::lock_guard<std::mutex> batch(r->multi_mu);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t G = r->parts.size();
    for (size_t k = 0; k < G; ++k) {
        pss_reader::Part *p = r->parts[k];
        std::lock_guard<std::mutex> lk(p->mu);
        p->rq = rq;
        if (k) p->pending = true;
    }
    for (size_t k = 1; k < G; ++k) r->parts[k]->cv.notify_all();
    part_run(r->parts[0]);
    int rc = r->parts[0]->rc;
    std::string err = r->parts[0]->err;
    for (size_t k = 1; k < G; ++k) {
        pss_reader::Part *p = r->parts[k];
        std::unique_lock<std::mutex> lk(p->mu);
        p->cv.wait(lk, [&] { return !p->pending; });
        if (p->rc != PSS_OK && rc == PSS_OK) {
            rc = p->rc;
            err = p->err;
        }
    }
    if (rc != PSS_OK) {
        set_error("%s", err.c_str());
        return rc;
    }
    pss_search_stats st{};
    st.queries = nq;
    uint64_t E = 0, B = 0;
    for (pss_reader::Part *p : r->parts) {
        const pss_search_stats &ps = p->reader->last;
        st.hits += ps.hits;
        st.entries += ps.entries;
        st.result_bytes += ps.result_bytes;
        st.ms_device = std::max(st.ms_device, ps.ms_device);
        st.ms_interval = std::max(st.ms_interval, ps.ms_interval);
        st.route |= ps.route;
        E += p->res.n_entries;
        B += p->res.n_bytes;
    }
    out->nq = nq;
    out->qcount = static_cast<uint64_t *>(calloc(nq ? nq : 1, sizeof(uint64_t)));
    if (!out->qcount) return PSS_ENOMEM;
    if (rq.mode == SEARCH_COUNTS) {
        for (pss_reader::Part *p : r->parts)
            for (uint32_t q = 0; q < nq; ++q) out->qcount[q] += p->res.qcount[q];
    } else {
        // The merged result lives where a single-device result would: a block of the pinned pool when it is large (reused
        // from batch to batch -- a fresh malloc of hundreds of megabytes is page faults on every first touch), else malloc.
        PSS_TRY(alloc_host_result(out, E, B, !search_knobs().no_pinned_results));
        // Query-major, part-major inside a query.  Round 6: by several threads -- one pass over the counts finds where
        // every RANGE of queries starts (output entry, output byte, every part's cursor), then the ranges are merged
        // side by side (one thread took 0.2 s for the 14.7 M entries / 0.6 GB of the 15-chunk `lines` batch: six times the
        // search itself; tests/tools/multi_merge_perf.py).
        struct RangeStart {
            uint32_t q0;
            uint64_t e_out, b_out;
            std::vector<uint64_t> cursor;
        };
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        const uint32_t want = (E >= (1u << 18) || B >= ((uint64_t)32 << 20)) ? std::min<uint32_t>(16u, std::max(1u, hw / 2)) : 1u;
        const uint32_t R = std::max<uint32_t>(1u, std::min<uint32_t>(want, nq ? nq : 1u));
        std::vector<RangeStart> starts(R);
        {
            std::vector<uint64_t> cursor(G, 0);
            uint64_t e_out = 0, b_out = 0;
            uint32_t next = 0;
            for (uint32_t q = 0; q <= nq; ++q) {
                while (next < R && q == (uint32_t)((uint64_t)nq * next / R)) {
                    starts[next] = RangeStart{q, e_out, b_out, cursor};
                    ++next;
                }
                if (q == nq) break;
                for (size_t k = 0; k < G; ++k) {
                    const HostResult &pr = r->parts[k]->res;
                    const uint64_t c = pr.qcount[q];
                    if (!c) continue;
                    const uint64_t e0 = cursor[k], e1 = e0 + c;
                    e_out += c;
                    b_out += pr.offsets[e1] - pr.offsets[e0];
                    cursor[k] = e1;
                }
            }
            out->offsets[e_out] = b_out;      // (= E, B)
        }
        auto merge_range = [&](uint32_t i) {
            const uint32_t q0 = starts[i].q0, q1 = i + 1 < R ? starts[i + 1].q0 : nq;
            std::vector<uint64_t> cursor = starts[i].cursor;
            uint64_t e_out = starts[i].e_out, b_out = starts[i].b_out;
            for (uint32_t q = q0; q < q1; ++q) {
                for (size_t k = 0; k < G; ++k) {
                    const HostResult &pr = r->parts[k]->res;
                    const uint64_t c = pr.qcount[q];
                    if (!c) continue;
                    const uint64_t e0 = cursor[k], e1 = e0 + c;
                    const uint64_t b0 = pr.offsets[e0], b1 = pr.offsets[e1];
                    for (uint64_t e = e0; e < e1; ++e) out->offsets[e_out++] = b_out + (pr.offsets[e] - b0);
                    memcpy(out->bytes + b_out, pr.bytes + b0, (size_t)(b1 - b0));
                    b_out += b1 - b0;
                    cursor[k] = e1;
                    out->qcount[q] += c;
                }
            }
        };
        if (R == 1) {
            merge_range(0);
        } else {
            std::vector<std::thread> th;
            for (uint32_t i = 1; i < R; ++i) th.emplace_back(merge_range, i);
            merge_range(0);
            for (auto &t : th) t.join();
        }
        out->n_entries = E;
        out->n_bytes = B;
    }
    for (pss_reader::Part *p : r->parts) p->res.release();
    st.ms_host = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    r->last = st;
    return PSS_OK;
}

// A batch into a fresh pss_result that *out hands to the caller (or that is freed again when the batch fails).
int reader_batch_result(pss_reader *r, const SearchRequest &rq, pss_result **out)
{
    pss_result *res = new pss_result();
    const int rc = reader_batch(r, rq, &res->r);
    if (rc != PSS_OK) {
        pss_result_free(res);
        return rc;
    }
    *out = res;
    return PSS_OK;
}

// The counts of a batch (rq.mode is set here) into the caller's counters, one per row of the result.
int reader_batch_counts(pss_reader *r, SearchRequest rq, uint64_t *counts)
{
    rq.mode = SEARCH_COUNTS;
    HostResult res;
    const int rc = reader_batch(r, rq, &res);
    if (rc == PSS_OK && rq.rows()) memcpy(counts, res.qcount, (size_t)rq.rows() * sizeof(uint64_t));
    res.release();
    return rc;
}

}  // namespace

extern "C" int pss_reader_add_chunk_device(pss_reader *r, const void *d_text, const void *d_sa, uint32_t n)
{
    return guarded([&]() -> int {
        if (!r || (n && (!d_text || !d_sa))) return PSS_EINVAL;
        if (!r->parts.empty()) {
            set_error("pss_reader_add_chunk_device: not on a multi-device reader");
            return PSS_EINVAL;
        }
        if (n == 0) return PSS_OK;
        std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
        ChunkDesc cd{};
        pss_reader::Mem cm;
        PSS_TRY(reader_alloc_chunk(r, n, &cd, &cm));
        r->chunks.push_back(cd);
        r->mem.push_back(cm);
        r->file_index.push_back(r->file_index.empty() ? 0 : r->file_index.back() + 1);      // (a reader made by pss_reader_create: the resident index)
        PSS_HIP(hipMemcpyAsync(cm.text, d_text, n, hipMemcpyDeviceToDevice, r->ctx->stream));
        PSS_HIP(hipMemcpyAsync(cm.sa, d_sa, (size_t)n * 4, cm.sa_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               r->ctx->stream));
        PSS_TRY(reader_sample_chunk(r, cd));
        PSS_HIP(hipStreamSynchronize(r->ctx->stream));
        r->dirty = true;
        return reader_sync_descs(r);
    });
}

extern "C" int pss_reader_set_chunk_device(pss_reader *r, uint64_t index, const void *d_text, const void *d_sa,
                                           uint32_t n)
{
    return guarded([&]() -> int {
        if (!r || !d_text || !d_sa || n == 0 || index > r->chunks.size() || !r->parts.empty()) {
            set_error("pss_reader_set_chunk_device: bad arguments");
            return PSS_EINVAL;
        }
        std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
        if (index == r->chunks.size()) return pss_reader_add_chunk_device(r, d_text, d_sa, n);
        ChunkDesc &c = r->chunks[index];
        if (c.n != n) {   // different size: fresh allocation
            ChunkDesc fresh{};
            pss_reader::Mem fm;
            reader_free_mem(r->mem[index]);            // first: its HBM may be what the new one needs
            c = ChunkDesc{};                           // (an empty chunk if the allocation below fails)
            r->dirty = true;
            PSS_TRY(reader_alloc_chunk(r, n, &fresh, &fm));
            c = fresh;
            r->mem[index] = fm;
            r->dirty = true;
        }
        reader_drop_lines(r->mem[index]);              // the next call that asks for ids indexes the new text
        const pss_reader::Mem &cm = r->mem[index];
        PSS_HIP(hipMemcpyAsync(cm.text, d_text, n, hipMemcpyDeviceToDevice, r->ctx->stream));
        PSS_HIP(hipMemcpyAsync(cm.sa, d_sa, (size_t)n * 4, cm.sa_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                               r->ctx->stream));
        PSS_TRY(reader_sample_chunk(r, c));
        PSS_HIP(hipStreamSynchronize(r->ctx->stream));
        return reader_sync_descs(r);
    });
}

namespace {

// Moves the suffix array of resident chunk `index` between the two tiers (HBM <-> pinned host memory the kernels read
// over PCIe); the key samples stay in HBM either way.  `to_host` = evict, else promote.
int reader_move_sa(pss_reader *r, uint64_t index, bool to_host)
{
    if (index >= r->chunks.size()) {
        set_error("chunk %llu of %zu", (unsigned long long)index, r->chunks.size());
        return PSS_EINVAL;
    }
    std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
    PSS_HIP(hipSetDevice(r->device));
    ChunkDesc &c = r->chunks[index];
    pss_reader::Mem &m = r->mem[index];
    if (m.sa_host == to_host || c.n == 0) return PSS_OK;
    const size_t sa_bytes = round_up((size_t)c.n * 4 + 16, 8);
    const size_t sk_bytes = c.skeys ? sample_count(c.n, c.shift) * 8 : 0;
    hipStream_t s = r->ctx->stream;
    if (to_host) {
        void *host = nullptr, *sk = nullptr;
        hipError_t e = hipHostMalloc(&host, sa_bytes, hipHostMallocPortable);
        if (e == hipSuccess && sk_bytes) e = hipMalloc(&sk, sk_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (host) (void)hipHostFree(host);
            set_error("evict: no pinned host memory for the suffix array of chunk %llu: %s", (unsigned long long)index, hipGetErrorString(e));
            return PSS_ENOMEM;
        }
        PSS_HIP(hipMemcpyAsync(host, m.sa, (size_t)c.n * 4, hipMemcpyDeviceToHost, s));
        if (sk_bytes) PSS_HIP(hipMemcpyAsync(sk, c.skeys, sk_bytes, hipMemcpyDeviceToDevice, s));
        PSS_HIP(hipStreamSynchronize(s));
        (void)hipFree(m.sa);
        m.sa = host;
        m.skeys = sk;
        m.sa_host = true;
        m.hbm_bytes -= sa_bytes;
        m.host_bytes = sa_bytes;
        void *dp = nullptr;
        PSS_HIP(hipHostGetDevicePointer(&dp, host, 0));
        c.sa = static_cast<uint32_t *>(dp);
        c.skeys = static_cast<uint64_t *>(sk);
    } else {
        void *dev = nullptr;
        const hipError_t e = hipMalloc(&dev, sa_bytes + sk_bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_error("promote: no HBM for the suffix array of chunk %llu: %s", (unsigned long long)index, hipGetErrorString(e));
            return PSS_ENOMEM;
        }
        uint64_t *sk = sk_bytes ? reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(dev) + sa_bytes) : nullptr;
        PSS_HIP(hipMemcpyAsync(dev, m.sa, (size_t)c.n * 4, hipMemcpyHostToDevice, s));
        if (sk_bytes) PSS_HIP(hipMemcpyAsync(sk, c.skeys, sk_bytes, hipMemcpyDeviceToDevice, s));
        PSS_HIP(hipStreamSynchronize(s));
        (void)hipHostFree(m.sa);
        if (m.skeys) (void)hipFree(m.skeys);
        m.sa = dev;
        m.skeys = nullptr;
        m.sa_host = false;
        m.hbm_bytes += sa_bytes;
        m.host_bytes = 0;
        c.sa = static_cast<uint32_t *>(dev);
        c.skeys = sk;
    }
    r->dirty = true;
    return reader_sync_descs(r);
}

// ---- residency manager ----------------------------------------------------------------------------------------
bool reader_hbm_room(pss_reader *r, size_t bytes)
{
    if (const char *ev = knob("PSS_READER_HBM_BUDGET")) {
        uint64_t used = 0;
        for (const auto &x : r->mem) used += x.hbm_bytes;
        return used + bytes <= strtoull(ev, nullptr, 0);
    }
    size_t free_b = 0, total_b = 0;
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= bytes + kHbmReserve;
}

uint64_t *reader_hits_buffer(pss_reader *r)
{
    if (!r->auto_residency) return nullptr;
    bool host = false;
    for (size_t c = 0; c < r->mem.size(); ++c) host = host || (r->mem[c].sa_host && !(c < r->manual.size() && r->manual[c]));
    if (!host) return nullptr;          // everything (the manager may move) lives in HBM: nothing to decide, nothing to measure
    r->batch_hits.assign(r->chunks.size(), 0);
    return r->batch_hits.data();
}

// After a batch whose per-chunk hits are in r->batch_hits: decay, then at most one exchange.  Failures to move are not
// failures of the search: the tiers stay as they are.
void reader_note_batch(pss_reader *r)
{
    const size_t nc = r->chunks.size();
    if (r->batch_hits.size() != nc || nc == 0) return;
    r->heat.resize(nc, 0);
    r->last_touch.resize(nc, 0);
    r->batch_seq += 1;
    for (size_t c = 0; c < nc; ++c) {
        r->heat[c] = r->heat[c] / 2 + r->batch_hits[c];
        if (r->batch_hits[c]) r->last_touch[c] = r->batch_seq;
    }
    r->batch_hits.clear();
    size_t hot = nc, cold = nc;
    for (size_t c = 0; c < nc; ++c) {
        if (r->chunks[c].n == 0 || (c < r->manual.size() && r->manual[c])) continue;
        if (r->mem[c].sa_host) {
            if (hot == nc || r->heat[c] > r->heat[hot]) hot = c;
        } else if (cold == nc || r->heat[c] < r->heat[cold] ||
                   (r->heat[c] == r->heat[cold] && r->last_touch[c] < r->last_touch[cold])) {
            cold = c;
        }
    }
    if (hot == nc || r->heat[hot] < 16) return;
    const size_t need = round_up((size_t)r->chunks[hot].n * 4 + 16, 8) +
                        (r->chunks[hot].skeys ? sample_count(r->chunks[hot].n, r->chunks[hot].shift) * 8 : 0);
    const std::string keep = last_error();
    if (reader_hbm_room(r, need)) {
        if (reader_move_sa(r, hot, false) == PSS_OK) r->auto_moves += 1;
    } else if (cold != nc && r->heat[hot] > 2 * r->heat[cold]) {
        if (reader_move_sa(r, cold, true) == PSS_OK) {
            if (reader_move_sa(r, hot, false) == PSS_OK) r->auto_moves += 1;
            else (void)reader_move_sa(r, cold, false);       // no room after all: back as it was
        }
    }
    set_error("%s", keep.c_str());
}

int reader_move_any(pss_reader *r, uint64_t index, bool to_host)
{
    if (!r) return PSS_EINVAL;
    pss_reader *x = r;
    uint64_t at = index;
    if (!r->parts.empty()) {
        const uint64_t G = r->parts.size();  // chunk c of the file lives in part c % G at position c / G
        x = r->parts[index % G]->reader;
        at = index / G;
    }
    PSS_TRY(reader_move_sa(x, at, to_host));
    std::lock_guard<std::recursive_mutex> lk(x->ctx->mu);
    x->manual.resize(x->chunks.size(), 0);
    x->manual[at] = 1;                       // placed by hand: the residency manager leaves it where it is
    return PSS_OK;
}

}  // namespace

extern "C" int pss_reader_evict_chunk(pss_reader *r, uint64_t index)
{
    return guarded([&]() -> int { return reader_move_any(r, index, true); });
}
extern "C" int pss_reader_promote_chunk(pss_reader *r, uint64_t index)
{
    return guarded([&]() -> int { return reader_move_any(r, index, false); });
}

extern "C" int pss_reader_set_auto_residency(pss_reader *r, int32_t on)
{
    if (!r) return PSS_EINVAL;
    r->auto_residency = on != 0;
    r->manual.clear();                       // (switching the manager on again hands every chunk back to it)
    for (pss_reader::Part *p : r->parts) {
        p->reader->auto_residency = on != 0;
        p->reader->manual.clear();
    }
    return PSS_OK;
}

extern "C" int pss_reader_chunk_tiers(const pss_reader *r, uint8_t *tiers, uint64_t cap, uint64_t *auto_moves)
{
    if (!r) return PSS_EINVAL;
    uint64_t moves = r->auto_moves;
    if (r->parts.empty()) {
        for (size_t c = 0; c < r->mem.size() && c < cap; ++c)
            if (tiers) tiers[c] = r->mem[c].sa_host ? 1 : 0;
    } else {
        const uint64_t G = r->parts.size();      // chunk c of the file lives in part c % G at position c / G
        for (uint64_t g = 0; g < G; ++g) {
            const pss_reader *x = r->parts[g]->reader;
            moves += x->auto_moves;
            for (size_t k = 0; k < x->mem.size(); ++k) {
                const uint64_t c = (uint64_t)k * G + g;
                if (tiers && c < cap) tiers[c] = x->mem[k].sa_host ? 1 : 0;
            }
        }
    }
    if (auto_moves) *auto_moves = moves;
    return PSS_OK;
}

extern "C" uint64_t pss_reader_part_chunks(const pss_reader *r, uint64_t *counts, uint64_t cap)
{
    if (!r) return 0;
    if (r->parts.empty()) {
        if (counts && cap) counts[0] = r->chunks.size();
        return 1;
    }
    for (size_t g = 0; g < r->parts.size() && g < cap; ++g)
        if (counts) counts[g] = r->parts[g]->reader->chunks.size();
    return r->parts.size();
}

extern "C" uint64_t pss_reader_num_chunks(const pss_reader *r)
{
    if (!r) return 0;
    uint64_t nc = r->chunks.size();
    for (const pss_reader::Part *p : r->parts) nc += p->reader->chunks.size();
    return nc;
}

extern "C" int pss_reader_residency(const pss_reader *r, uint64_t *hbm_bytes, uint64_t *host_bytes, uint64_t *host_chunks)
{
    if (!r) return PSS_EINVAL;
    uint64_t hb = 0, pb = 0, hc = 0;
    auto add = [&](const pss_reader *x) {
        for (const auto &m : x->mem) {
            hb += m.hbm_bytes;
            pb += m.host_bytes;
            hc += m.sa_host ? 1 : 0;
        }
    };
    add(r);
    for (const pss_reader::Part *p : r->parts) add(p->reader);
    if (hbm_bytes) *hbm_bytes = hb;
    if (host_bytes) *host_bytes = pb;
    if (host_chunks) *host_chunks = hc;
    return PSS_OK;
}

extern "C" int pss_reader_search_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                       pss_result **out)
{
    return guarded([&]() -> int {
        if (!r || !out || (nq && !qoffsets)) {
            set_error("pss_reader_search_batch: bad arguments");
            return PSS_EINVAL;
        }
        return reader_batch_result(r, SearchRequest{qbytes, qoffsets, nq}, out);
    });
}

extern "C" int pss_reader_set_low_latency(pss_reader *r, int32_t on)
{
    return guarded([&]() -> int {
        if (!r || !r->parts.empty()) {
            set_error("pss_reader_set_low_latency: a single-device reader is required");
            return PSS_EINVAL;
        }
        std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
        PSS_HIP(hipSetDevice(r->device));
        r->low_latency = on != 0;
        if (!on) r->ctx->stop_resident();
        return PSS_OK;
    });
}

extern "C" int pss_reader_set_result_order(pss_reader *r, int32_t order)
{
    return guarded([&]() -> int {
        if (!r || (order != PSS_ORDER_TEXT && order != PSS_ORDER_SA)) {
            set_error("pss_reader_set_result_order: bad arguments");
            return PSS_EINVAL;
        }
        r->order_sa = order == PSS_ORDER_SA;
        for (auto *p : r->parts) p->reader->order_sa = r->order_sa;
        return PSS_OK;
    });
}

extern "C" int32_t pss_reader_result_order(const pss_reader *r) { return (r && r->order_sa) ? PSS_ORDER_SA : PSS_ORDER_TEXT; }

extern "C" int pss_reader_low_latency_stats(const pss_reader *r, uint64_t *launches, uint64_t *served)
{
    if (!r || !r->ctx) return PSS_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(r->ctx->mu);
    if (launches) *launches = r->ctx->resident.launches;
    if (served) *served = r->ctx->resident.served;
    return PSS_OK;
}

extern "C" int pss_reader_count_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                      uint64_t *counts)
{
    return guarded([&]() -> int {
        if (!r || (nq && (!qoffsets || !counts))) {
            set_error("pss_reader_count_batch: bad arguments");
            return PSS_EINVAL;
        }
        return reader_batch_counts(r, SearchRequest{qbytes, qoffsets, nq}, counts);
    });
}

extern "C" int pss_reader_search_batch_device(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                              pss_device_result *out)
{
    return guarded([&]() -> int {
        if (!r || !out || (nq && !qoffsets)) {
            set_error("pss_reader_search_batch_device: bad arguments");
            return PSS_EINVAL;
        }
        if (!r->parts.empty()) {
            set_error("pss_reader_search_batch_device: a multi-device reader has no single device to leave the result on");
            return PSS_EINVAL;
        }
        HostResult hr;
        const int rc = reader_batch(r, SearchRequest{qbytes, qoffsets, nq, SEARCH_DEVICE}, &hr);
        if (rc == PSS_OK) {
            out->num_queries = nq;
            out->num_entries = hr.n_entries;
            out->num_bytes = hr.n_bytes;
            out->d_counts = hr.d_qcount;
            out->d_offsets = hr.d_offsets;
            out->d_bytes = hr.d_bytes;
            out->device = r->device;
        }
        hr.release();
        return rc;
    });
}

// ---- entry ids ---------------------------------------------------------------------------------------------------

extern "C" int pss_reader_search_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                           pss_result **out)
{
    return guarded([&]() -> int {
        if (!r || !out || (nq && !qoffsets)) {
            set_error("pss_reader_search_ids_batch: bad arguments");
            return PSS_EINVAL;
        }
        // (on a multi-device reader the parts' ids travel as the bytes of ordinary packed results, 8 per entry: the merge is the
        // one of the entries)
        return reader_batch_result(r, SearchRequest{qbytes, qoffsets, nq, SEARCH_IDS}, out);
    });
}

// ---- what the entry points of the anchored, group and seeded batches share -----------------------------------------

namespace {

// The common end of those calls: the batch's answer by mode -- its counts, or its result.
int answer_by_mode(pss_reader *r, const SearchRequest &rq, pss_result **out, uint64_t *counts)
{
    return rq.mode == SEARCH_COUNTS ? reader_batch_counts(r, rq, counts) : reader_batch_result(r, rq, out);
}

// Is the output argument that the mode asks for usable?  (No row: the counts may be null.)
bool out_ok_by_mode(SearchMode mode, uint32_t rows, pss_result **out, const uint64_t *counts)
{
    return mode == SEARCH_COUNTS ? !rows || counts : out != nullptr;
}

// The offsets of a batch of plain patterns: they start at 0 and do not decrease, and no pattern is empty or has more than
// 2^32 - 1 bytes.  each(q, len) is the batch's own check of pattern q, made once q is known non-empty; it states its own
// error.
template <typename Each>
int pattern_args(const char *who, const uint64_t *qoffsets, uint32_t nq, Each each)
{
    if (nq && qoffsets[0] != 0) {
        set_error("%s: the pattern offsets start at %llu, not at 0", who, (unsigned long long)qoffsets[0]);
        return PSS_EINVAL;
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (qoffsets[q + 1] < qoffsets[q]) {
            set_error("%s: the pattern offsets decrease at pattern %u", who, q);
            return PSS_EINVAL;
        }
        const uint64_t len = qoffsets[q + 1] - qoffsets[q];
        if (len == 0) {
            set_error("%s: pattern %u is empty (every entry contains the empty pattern)", who, q);
            return PSS_EINVAL;
        }
        if (!each(q, len)) return PSS_EINVAL;
        if (len > 0xffffffffull) {
            set_error("%s: pattern %u has more than 2^32 - 1 bytes (a chunk has fewer)", who, q);
            return PSS_EINVAL;
        }
    }
    return PSS_OK;
}

uint32_t icase_letters(int32_t letters) { return letters <= 0 ? search_knobs().icase_seed_letters : (uint32_t)letters; }

// The terms of a seeded batch (search.h) as the interval search takes them: the seed queries of every term back to back
// (the spellings of its seed, or its pieces), the offsets that say which queries are whose, and the position of every
// query inside its term; under fold beside them the terms folded to lower case.  A batch of plain patterns adds its groups
// of one include term each: identity offsets and zero exclude flags.  It lives in the entry point's frame, so it outlives
// the batch on every part of a multi-device reader.
struct SeededGroups {
    std::vector<uint8_t> vbytes, fbytes, no_exclude;
    std::vector<uint64_t> voff, soff, foff, one_each;
    std::vector<uint32_t> pos;
    void one_term_each(uint32_t n)
    {
        one_each.resize((size_t)n + 1);
        for (uint64_t g = 0; g <= n; ++g) one_each[g] = g;
        no_exclude.assign((size_t)n + 1, 0);
    }
    // (the terms as they are verified: the folded ones; a near batch puts its patterns and budgets in their place)
    SearchRequest request(uint32_t nterms, const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, const uint8_t *anchors,
                          SearchMode mode) const
    {
        SearchRequest rq{vbytes.data(), voff.data(), (uint32_t)(voff.size() - 1), mode, nullptr, group_offsets, ngroups, exclude, anchors};
        rq.term_bytes = fbytes.data();
        rq.term_offsets = foff.data();
        rq.nterms = nterms;
        rq.seed_offsets = soff.data();
        rq.seed_pos = pos.data();
        return rq;
    }
};

// The expansion of n terms (`noun`: "pattern", "term" or "segment") that pattern_args / terms_args / seq_args have passed:
// every one non-empty.  What it holds is judged before anything is allocated for it.  At most 64 spellings per term: only a
// batch of more than 2^26 terms can pass the limit, and only such a batch pays for a counting pass of its own.
int icase_expand(const char *who, const char *noun, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t n, SeededGroups *b)
{
    const uint32_t letters = icase_letters(0);
    for (uint32_t t = 0; t < n; ++t)
        if (toffsets[t + 1] - toffsets[t] > 0xffffffffull) {
            set_error("%s: %s %u has more than 2^32 - 1 bytes (a chunk has fewer)", who, noun, t);
            return PSS_EINVAL;
        }
    if (((uint64_t)n << letters) > 0xffffffffull) {
        uint64_t count = 0;
        for (uint32_t t = 0; t < n; ++t) {
            uint64_t so = 0, sl = 0;
            count += 1ull << fold_seed(tbytes + toffsets[t], toffsets[t + 1] - toffsets[t], letters, &so, &sl);
            if (count > 0xffffffffull) {
                set_error("%s: the %ss expand to more than the 2^32 - 1 terms an all-terms batch takes (at %s %u)", who, noun, noun, t);
                return PSS_EINVAL;
            }
        }
    }
    std::vector<uint64_t> slen(n);
    std::vector<uint32_t> seed(n);
    std::vector<uint8_t> nletters(n);
    uint64_t nspell = 0, vtotal = 0, ftotal = 0;
    for (uint32_t t = 0; t < n; ++t) {
        const uint64_t len = toffsets[t + 1] - toffsets[t];
        uint64_t so = 0;
        nletters[t] = (uint8_t)fold_seed(tbytes + toffsets[t], len, letters, &so, &slen[t]);
        nspell += 1ull << nletters[t];
        vtotal += slen[t] << nletters[t];
        ftotal += len;
        seed[t] = (uint32_t)so;             // (inside a term of less than 2^32 bytes)
    }
    b->fbytes.resize(ftotal + 1);
    b->vbytes.resize(vtotal + 1);
    b->voff.reserve(nspell + 1);
    b->pos.reserve(nspell + 1);
    b->soff.reserve((size_t)n + 1);
    b->foff.reserve((size_t)n + 1);
    b->voff.assign(1, 0);
    b->soff.assign(1, 0);
    b->foff.assign(1, 0);
    for (uint32_t t = 0; t < n; ++t) {
        const uint8_t *src = tbytes + toffsets[t];
        const uint64_t len = toffsets[t + 1] - toffsets[t];
        uint8_t *dst = b->fbytes.data() + b->foff.back();
        for (uint64_t i = 0; i < len; ++i) dst[i] = (uint8_t)((uint8_t)(src[i] - 'A') < 26 ? src[i] | 0x20 : src[i]);
        b->foff.push_back(b->foff.back() + len);
        const uint32_t f = nletters[t];
        fold_spellings(src + seed[t], slen[t], f, b->vbytes.data() + b->voff.back());
        for (uint32_t v = 0; v < (1u << f); ++v) {          // (every spelling stands where the seed stands)
            b->voff.push_back(b->voff.back() + slen[t]);
            b->pos.push_back(seed[t]);
        }
        b->soff.push_back(b->soff.back() + (1ull << f));
    }
    b->pos.push_back(0);                    // (data() of an empty vector may be null)
    return PSS_OK;
}

}  // namespace

// ---- anchored search (anchored_impl.h) ---------------------------------------------------------------------------

namespace {

// The argument checks of the three anchored calls (out_ok: the call's own output argument is usable).
int anchored_args(const pss_reader *r, const char *who, const uint64_t *qoffsets, uint32_t nq, const uint8_t *anchors, bool out_ok)
{
    if (!r || !out_ok || (nq && (!qoffsets || !anchors))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    for (uint32_t q = 0; q < nq; ++q)
        if (anchors[q] == 0 || anchors[q] > (PSS_ANCHOR_START | PSS_ANCHOR_END)) {
            set_error("%s: anchors[%u] = %u (PSS_ANCHOR_START = 1, PSS_ANCHOR_END = 2 or both; an unanchored batch is pss_reader_search_batch's)",
                      who, q, (unsigned)anchors[q]);
            return PSS_EINVAL;
        }
    return PSS_OK;
}

int anchored_batch(pss_reader *r, const char *who, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *anchors,
                   SearchMode mode, pss_result **out, uint64_t *counts)
{
    PSS_TRY(anchored_args(r, who, qoffsets, nq, anchors, out_ok_by_mode(mode, nq, out, counts)));
    return answer_by_mode(r, SearchRequest{qbytes, qoffsets, nq, mode, anchors}, out, counts);
}

}  // namespace

extern "C" int pss_reader_search_anchored_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return anchored_batch(r, "pss_reader_search_anchored_batch", qbytes, qoffsets, nq, anchors, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_anchored_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                    const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return anchored_batch(r, "pss_reader_search_anchored_ids_batch", qbytes, qoffsets, nq, anchors, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_anchored_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                               const uint8_t *anchors, uint64_t *counts)
{
    return guarded([&]() -> int { return anchored_batch(r, "pss_reader_count_anchored_batch", qbytes, qoffsets, nq, anchors, SEARCH_COUNTS, nullptr, counts); });
}

// ---- all-terms search (all_terms_impl.h), plain and case-insensitive (group -> terms -> spellings) ------

namespace {

// The group offsets of an all-terms or a sequence batch against its n members (`noun`: "terms" or "segments"): they run
// from 0 to n and never decrease.  group_ok(g) is the batch's own check of group g, made once g's offsets are known good;
// it states its own error.  The reader is looked at last, as pss.h says: a malformed batch is reported as such with or
// without one.
template <typename GroupOk>
int group_args(const pss_reader *r, const char *who, const char *noun, const uint64_t *group_offsets, uint32_t ngroups, uint32_t n,
               GroupOk group_ok)
{
    if (group_offsets[0] != 0 || group_offsets[ngroups] != n) {
        set_error("%s: the group offsets run from %llu to %llu, not from 0 to the %u %s", who, (unsigned long long)group_offsets[0],
                  (unsigned long long)group_offsets[ngroups], n, noun);
        return PSS_EINVAL;
    }
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (group_offsets[g + 1] < group_offsets[g] || group_offsets[g + 1] > n) {
            set_error("%s: the group offsets decrease or pass the %u %s at group %u", who, n, noun, g);
            return PSS_EINVAL;
        }
        if (!group_ok(g)) return PSS_EINVAL;
    }
    if (!r) {
        set_error("%s: bad arguments (no reader)", who);
        return PSS_EINVAL;
    }
    return PSS_OK;
}

// The argument checks of the three all-terms calls (out_ok: the call's own output argument is usable).
int terms_args(const pss_reader *r, const char *who, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms,
               const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *exclude, bool out_ok)
{
    if (!out_ok || !group_offsets || (nterms && (!tbytes || !toffsets || !exclude))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    for (uint32_t t = 0; t < nterms; ++t) {
        if (toffsets[t + 1] <= toffsets[t]) {
            set_error("%s: term %u is empty (every entry contains the empty term: leave it out)", who, t);
            return PSS_EINVAL;
        }
        if (exclude[t] > 1) {
            set_error("%s: exclude[%u] = %u (0 = the entry must contain the term, 1 = it must not)", who, t, (unsigned)exclude[t]);
            return PSS_EINVAL;
        }
    }
    return group_args(r, who, "terms", group_offsets, ngroups, nterms, [&](uint32_t g) {
        bool include = false;
        for (uint64_t t = group_offsets[g]; t < group_offsets[g + 1] && !include; ++t) include = exclude[t] == 0;
        if (!include) set_error("%s: group %u has no include term (\"everything except\" is not a search)", who, g);
        return include;
    });
}

// The six all-terms calls: the argument checks, then the batch as it stands or, under icase, expanded into its seeds'
// spellings.
int terms_batch(pss_reader *r, const char *who, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
                uint32_t ngroups, const uint8_t *exclude, bool icase, SearchMode mode, pss_result **out, uint64_t *counts)
{
    PSS_TRY(terms_args(r, who, tbytes, toffsets, nterms, group_offsets, ngroups, exclude, out_ok_by_mode(mode, ngroups, out, counts)));
    if (!icase) return answer_by_mode(r, SearchRequest{tbytes, toffsets, nterms, mode, nullptr, group_offsets, ngroups, exclude}, out, counts);
    SeededGroups b;
    PSS_TRY(icase_expand(who, "term", tbytes, toffsets, nterms, &b));
    return answer_by_mode(r, b.request(nterms, group_offsets, ngroups, exclude, nullptr, mode), out, counts);
}

}  // namespace

extern "C" int pss_reader_search_terms_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, pss_result **out)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_search_terms_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, false, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_terms_ids_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, pss_result **out)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_search_terms_ids_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, false, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_terms_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, uint64_t *counts)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_count_terms_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, false, SEARCH_COUNTS, nullptr, counts); });
}

// ---- wildcard search: segments in order (sequence_impl.h), plain and case-insensitive ------------------------------

namespace {

// What the sequence calls and the class calls ask of segment t and of group g alike; each states its own error.
bool segment_ok(const char *who, const uint64_t *soffsets, uint32_t t)
{
    if (soffsets[t + 1] > soffsets[t]) return true;
    set_error("%s: segment %u is empty (two wildcards in a row are one: leave it out)", who, t);
    return false;
}
bool seq_group_ok(const char *who, const uint64_t *group_offsets, const uint8_t *anchors, uint32_t g)
{
    if (group_offsets[g + 1] == group_offsets[g]) {
        set_error("%s: group %u has no segment (a pattern of wildcards alone is not a search)", who, g);
        return false;
    }
    if (anchors[g] > (PSS_ANCHOR_START | PSS_ANCHOR_END)) {
        set_error("%s: anchors[%u] = %u (0, PSS_ANCHOR_START = 1, PSS_ANCHOR_END = 2 or both)", who, g, (unsigned)anchors[g]);
        return false;
    }
    return true;
}

// The argument checks of the three sequence calls (out_ok: the call's own output argument is usable).
int seq_args(const pss_reader *r, const char *who, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs,
             const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, bool out_ok)
{
    if (!out_ok || !group_offsets || !anchors || (nsegs && (!sbytes || !soffsets))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    for (uint32_t t = 0; t < nsegs; ++t)
        if (!segment_ok(who, soffsets, t)) return PSS_EINVAL;
    return group_args(r, who, "segments", group_offsets, ngroups, nsegs, [&](uint32_t g) { return seq_group_ok(who, group_offsets, anchors, g); });
}

// The six sequence calls, as terms_batch: group -> segments, under icase -> spellings.
int seq_batch(pss_reader *r, const char *who, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
              uint32_t ngroups, const uint8_t *anchors, bool icase, SearchMode mode, pss_result **out, uint64_t *counts)
{
    PSS_TRY(seq_args(r, who, sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, out_ok_by_mode(mode, ngroups, out, counts)));
    if (!icase)
        return answer_by_mode(r, SearchRequest{sbytes, soffsets, nsegs, mode, nullptr, group_offsets, ngroups, nullptr, anchors}, out, counts);
    SeededGroups b;
    PSS_TRY(icase_expand(who, "segment", sbytes, soffsets, nsegs, &b));
    return answer_by_mode(r, b.request(nsegs, group_offsets, ngroups, nullptr, anchors, mode), out, counts);
}

}  // namespace

extern "C" int pss_reader_search_seq_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_search_seq_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, false, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_seq_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_search_seq_ids_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, false, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_seq_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, uint64_t *counts)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_count_seq_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, false, SEARCH_COUNTS, nullptr, counts); });
}

// ---- wildcard search with byte classes: segments of literals, `?` and `[...]` (seq_class_impl.h) ------

namespace {

// The core of one segment from its class plane: offset and length of the longest run of literal positions (plane 0), the
// leftmost on a tie; length 0 for a segment without a literal position.  The rule of glob_cores in the Python layer.
void segment_core(const uint8_t *plane, uint64_t len, uint32_t *off, uint32_t *clen)
{
    uint64_t best_off = 0, best_len = 0;
    for (uint64_t i = 0; i < len;) {
        if (plane[i]) {
            ++i;
            continue;
        }
        uint64_t j = i;
        while (j < len && !plane[j]) ++j;
        if (j - i > best_len) {
            best_off = i;
            best_len = j - i;
        }
        i = j;
    }
    *off = (uint32_t)best_off;
    *clen = (uint32_t)best_len;
}

bool set_has(const uint8_t *set, uint32_t b) { return (set[b >> 3] >> (b & 7)) & 1u; }

// The sets of a class batch: none empty, none with 0x0A, under fold every one closed under it.
int seqc_sets_ok(const char *who, const uint8_t *sets, uint32_t nsets, bool fold)
{
    for (uint32_t k = 0; k < nsets; ++k) {
        const uint8_t *set = sets + (size_t)k * 32;
        bool any = false;
        for (uint32_t w = 0; w < 32; ++w) any = any || set[w];
        if (!any) {
            set_error("%s: set %u is empty (no byte of an entry is in it)", who, k + 1);
            return PSS_EINVAL;
        }
        if (set_has(set, 0x0A)) {
            set_error("%s: set %u holds 0x0A (no entry holds a newline: leave it out)", who, k + 1);
            return PSS_EINVAL;
        }
        for (uint32_t b = 'A'; fold && b <= 'Z'; ++b)
            if (set_has(set, b) != set_has(set, b | 0x20)) {
                set_error("%s: set %u holds one case of '%c' alone: under PSS_SEQ_FOLD a set is closed under the fold", who, k + 1, (int)b);
                return PSS_EINVAL;
            }
    }
    return PSS_OK;
}

// The walk over the segments of a class batch: every check of a segment's positions, its core into cores[2 t], cores[2 t + 1]
// (class_cores of the request) and newline[t] = it holds a literal 0x0A.
int seqc_segments(const char *who, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs, const uint8_t *sets,
                  uint32_t nsets, uint32_t *cores, uint8_t *newline)
{
    for (uint32_t t = 0; t < nsegs; ++t) {
        if (!segment_ok(who, soffsets, t)) return PSS_EINVAL;
        const uint64_t len = soffsets[t + 1] - soffsets[t];
        if (len > 0xffffffffull) {
            set_error("%s: segment %u has more than 2^32 - 1 bytes (a chunk has fewer)", who, t);
            return PSS_EINVAL;
        }
        const uint8_t *sb = sbytes + soffsets[t], *sp = classes + soffsets[t];
        bool all_any = true;
        for (uint64_t i = 0; i < len; ++i) {
            if (sp[i] > nsets) {
                set_error("%s: segment %u names set %u at position %llu, and the batch has %u", who, t, (unsigned)sp[i], (unsigned long long)i, nsets);
                return PSS_EINVAL;
            }
            if (sp[i] && sb[i]) {
                set_error("%s: segment %u holds the byte %#x under a class index at position %llu (a class position's byte is 0)", who, t,
                          (unsigned)sb[i], (unsigned long long)i);
                return PSS_EINVAL;
            }
            if (!sp[i] && sb[i] == '\n') newline[t] = 1;
            if (sp[i]) {                                    // (every byte but 0x0A: what `?` stands for)
                const uint8_t *set = sets + (size_t)(sp[i] - 1) * 32;
                for (uint32_t w = 0; w < 32 && all_any; ++w) all_any = set[w] == (w == 1 ? 0xfb : 0xff);
            }
        }
        segment_core(sp, len, &cores[2 * (size_t)t], &cores[2 * (size_t)t + 1]);
        if (!cores[2 * (size_t)t + 1]) cores[2 * (size_t)t] = all_any ? 1u : 0u;
    }
    return PSS_OK;
}

// The cores as the terms of a sequence batch: their bytes back to back (as the caller wrote them: the expansion folds),
// offsets, groups, void flags (a group with a literal 0x0A somewhere matches nothing).
struct CoreTerms {
    std::vector<uint8_t> bytes, dead;
    std::vector<uint64_t> off{0}, goff{0};
    uint32_t n = 0;
    CoreTerms(const uint8_t *sbytes, const uint64_t *soffsets, const uint64_t *group_offsets, uint32_t ngroups, const uint32_t *cores,
              const uint8_t *newline)
    {
        for (uint32_t g = 0; g < ngroups; ++g) {
            bool dead_group = false;
            for (uint64_t t = group_offsets[g]; t < group_offsets[g + 1]; ++t) dead_group = dead_group || newline[t];
            for (uint64_t t = group_offsets[g]; t < group_offsets[g + 1]; ++t) {
                const uint32_t co = cores[2 * t], cl = cores[2 * t + 1];
                if (!cl) continue;
                bytes.insert(bytes.end(), sbytes + soffsets[t] + co, sbytes + soffsets[t] + co + cl);
                off.push_back(bytes.size());
                dead.push_back(dead_group ? 1 : 0);
            }
            goff.push_back(off.size() - 1);
        }
        n = (uint32_t)(off.size() - 1);
        bytes.push_back(0);                 // (data() of an empty vector may be null)
        dead.push_back(0);
    }
};

// The three class calls: the argument checks -- every one a sequence call makes, then the class plane's and the sets' --, the
// cores of the segments as the terms of a sequence batch, under PSS_SEQ_FOLD expanded into their seeds' spellings, and the
// segments themselves in the request's class block.  The batch is judged before the reader is, as everywhere.
int seqc_batch(pss_reader *r, const char *who, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
               const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint32_t flags,
               SearchMode mode, pss_result **out, uint64_t *counts)
{
    if (!out_ok_by_mode(mode, ngroups, out, counts) || !group_offsets || !anchors || (nsegs && (!sbytes || !classes || !soffsets)) ||
        (nsets && !sets)) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    if (flags & ~PSS_SEQ_FOLD) {
        set_error("%s: flags = %#x (0 or PSS_SEQ_FOLD)", who, (unsigned)flags);
        return PSS_EINVAL;
    }
    if (nsets > 255) {
        set_error("%s: %u sets (the class plane names a set in one byte: 255 at most)", who, nsets);
        return PSS_EINVAL;
    }
    const bool fold = (flags & PSS_SEQ_FOLD) != 0;
    PSS_TRY(seqc_sets_ok(who, sets, nsets, fold));
    std::vector<uint32_t> cores((size_t)nsegs * 2 + 2);
    std::vector<uint8_t> newline((size_t)nsegs + 1);
    PSS_TRY(seqc_segments(who, sbytes, classes, soffsets, nsegs, sets, nsets, cores.data(), newline.data()));
    PSS_TRY(group_args(r, who, "segments", group_offsets, ngroups, nsegs, [&](uint32_t g) {
        if (!seq_group_ok(who, group_offsets, anchors, g)) return false;
        bool cored = false;
        for (uint64_t t = group_offsets[g]; t < group_offsets[g + 1] && !cored; ++t) cored = cores[2 * t + 1] != 0;
        if (!cored) set_error("%s: group %u has no segment with a literal byte: nothing in the suffix array can be looked up for it", who, g);
        return cored;
    }));
    const CoreTerms c(sbytes, soffsets, group_offsets, ngroups, cores.data(), newline.data());
    std::vector<uint8_t> fbytes;
    const uint8_t *seg_bytes = sbytes;
    if (fold) {                             // (the literals as they are compared: lower case; a class position's 0 stays)
        fbytes.assign(sbytes, sbytes + (nsegs ? soffsets[nsegs] : 0));
        for (uint8_t &b : fbytes)
            if ((uint8_t)(b - 'A') < 26) b |= 0x20;
        fbytes.push_back(0);
        seg_bytes = fbytes.data();
    }
    SeededGroups b;
    SearchRequest rq{c.bytes.data(), c.off.data(), c.n, mode, nullptr, c.goff.data(), ngroups, nullptr, anchors};
    if (fold) {
        PSS_TRY(icase_expand(who, "core", c.bytes.data(), c.off.data(), c.n, &b));
        rq = b.request(c.n, c.goff.data(), ngroups, nullptr, anchors, mode);
    }
    rq.class_bytes = seg_bytes;
    rq.class_plane = classes;
    rq.class_offsets = soffsets;
    rq.class_nsegs = nsegs;
    rq.class_groups = group_offsets;
    rq.class_cores = cores.data();
    rq.class_sets = sets;
    rq.class_nsets = nsets;
    rq.class_void = c.dead.data();
    return answer_by_mode(r, rq, out, counts);
}

}  // namespace

extern "C" int pss_reader_search_seqc_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
        const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint32_t flags, pss_result **out)
{
    return guarded([&]() -> int { return seqc_batch(r, "pss_reader_search_seqc_batch", sbytes, classes, soffsets, nsegs, sets, nsets, group_offsets, ngroups, anchors, flags, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_seqc_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
        const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint32_t flags, pss_result **out)
{
    return guarded([&]() -> int { return seqc_batch(r, "pss_reader_search_seqc_ids_batch", sbytes, classes, soffsets, nsegs, sets, nsets, group_offsets, ngroups, anchors, flags, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_seqc_batch(pss_reader *r, const uint8_t *sbytes, const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs,
        const uint8_t *sets, uint32_t nsets, const uint64_t *group_offsets, uint32_t ngroups, const uint8_t *anchors, uint32_t flags, uint64_t *counts)
{
    return guarded([&]() -> int { return seqc_batch(r, "pss_reader_count_seqc_batch", sbytes, classes, soffsets, nsegs, sets, nsets, group_offsets, ngroups, anchors, flags, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_seqc_cores(const uint8_t *classes, const uint64_t *soffsets, uint32_t nsegs, uint32_t *core_off, uint32_t *core_len)
{
    return guarded([&]() -> int {
        if (nsegs && (!classes || !soffsets || !core_off || !core_len)) {
            set_error("pss_seqc_cores: bad arguments");
            return PSS_EINVAL;
        }
        for (uint32_t t = 0; t < nsegs; ++t) {
            if (soffsets[t + 1] < soffsets[t] || soffsets[t + 1] - soffsets[t] > 0xffffffffull) {
                set_error("pss_seqc_cores: the segment offsets decrease at segment %u, or it has more than 2^32 - 1 bytes", t);
                return PSS_EINVAL;
            }
            segment_core(classes + soffsets[t], soffsets[t + 1] - soffsets[t], &core_off[t], &core_len[t]);
        }
        return PSS_OK;
    });
}

// ---- regular-expression search: pattern -> its required literals as an all-terms group + its DFA (regex_compile.h, -----
// ---- regex_impl.h) -----------------------------------------------------------------------------------

struct pss_regex {
    RegexDfa dfa;
};

namespace {

// One pattern compiled, its refusal stated as the entry point's (g < 0: the call has one pattern and names none).
int regex_compile_as(const char *who, int64_t g, const uint8_t *pat, uint64_t len, uint32_t flags, RegexDfa *d)
{
    std::string why;
    if (regex_compile(pat, len, flags, d, &why)) return PSS_OK;
    if (g < 0)
        set_error("%s: %s", who, why.c_str());
    else
        set_error("%s: pattern %lld: %s", who, (long long)g, why.c_str());
    return PSS_EINVAL;
}

// The three regex calls: arguments, then the patterns -- each compiled, its required literals the include terms of its
// group, its header, class map and table behind those of the patterns before it --, the reader last (terms_args).  Under
// PSS_REGEX_ICASE the literals (folded already) are expanded into their seeds' spellings as a case-insensitive all-terms
// batch expands its terms.  Everything lives in this frame, so it outlives the batch on every part of a multi-device reader.
int regex_batch(pss_reader *r, const char *who, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                SearchMode mode, pss_result **out, uint64_t *counts)
{
    if (!out_ok_by_mode(mode, np, out, counts) || (np && (!pbytes || !poffsets))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    if (flags & ~PSS_REGEX_ICASE) {
        set_error("%s: flags = %u (PSS_REGEX_ICASE = 1 or nothing)", who, flags);
        return PSS_EINVAL;
    }
    if (np && poffsets[0] != 0) {
        set_error("%s: the pattern offsets start at %llu, not at 0", who, (unsigned long long)poffsets[0]);
        return PSS_EINVAL;
    }
    for (uint32_t g = 0; g < np; ++g)
        if (poffsets[g + 1] < poffsets[g]) {
            set_error("%s: the pattern offsets decrease at pattern %u", who, g);
            return PSS_EINVAL;
        }
    std::vector<uint8_t> tbytes, cls;
    std::vector<uint64_t> toffsets(1, 0), goff(1, 0);
    std::vector<uint32_t> hdr;
    std::vector<uint16_t> tables;
    for (uint32_t g = 0; g < np; ++g) {
        RegexDfa d;
        PSS_TRY(regex_compile_as(who, g, pbytes + poffsets[g], poffsets[g + 1] - poffsets[g], flags, &d));
        if ((tables.size() + d.table.size()) * 2 > REGEX_MAX_TABLE_BYTES) {
            set_error("%s: the tables of the batch pass 64 MiB at pattern %u: split the batch", who, g);
            return PSS_EINVAL;
        }
        for (const std::string &lit : d.literals) {
            tbytes.insert(tbytes.end(), lit.begin(), lit.end());
            toffsets.push_back(tbytes.size());
        }
        goff.push_back(toffsets.size() - 1);
        const uint32_t h[REGEX_HDR_WORDS] = {(uint32_t)tables.size(), d.nstates, d.ncls, d.start, d.first_accept, d.sink, d.anchors, 0};
        hdr.insert(hdr.end(), h, h + REGEX_HDR_WORDS);
        cls.insert(cls.end(), d.cls, d.cls + 256);
        tables.insert(tables.end(), d.table.begin(), d.table.end());
    }
    const uint32_t nterms = (uint32_t)(toffsets.size() - 1);        // (at most 8 per pattern)
    tbytes.push_back(0);                                            // (data() of an empty vector may be null)
    const std::vector<uint8_t> no_exclude((size_t)nterms + 1, 0);
    PSS_TRY(terms_args(r, who, tbytes.data(), toffsets.data(), nterms, goff.data(), np, no_exclude.data(), true));
    SeededGroups b;
    SearchRequest rq{tbytes.data(), toffsets.data(), nterms, mode, nullptr, goff.data(), np, no_exclude.data()};
    if (flags & PSS_REGEX_ICASE) {
        PSS_TRY(icase_expand(who, "literal", tbytes.data(), toffsets.data(), nterms, &b));
        rq = b.request(nterms, goff.data(), np, no_exclude.data(), nullptr, mode);
    }
    if (np) {
        rq.regex_hdr = hdr.data();
        rq.regex_cls = cls.data();
        rq.regex_tables = tables.data();
        rq.regex_table_words = tables.size();
    }
    return answer_by_mode(r, rq, out, counts);
}

}  // namespace

extern "C" int pss_regex_compile(const uint8_t *pattern, uint64_t len, uint32_t flags, pss_regex **out)
{
    return guarded([&]() -> int {
        if (!out || (len && !pattern) || (flags & ~PSS_REGEX_ICASE)) {
            set_error("pss_regex_compile: bad arguments");
            return PSS_EINVAL;
        }
        std::unique_ptr<pss_regex> rx(new pss_regex);
        PSS_TRY(regex_compile_as("pss_regex_compile", -1, pattern, len, flags, &rx->dfa));
        *out = rx.release();
        return PSS_OK;
    });
}

extern "C" void pss_regex_free(pss_regex *rx) { delete rx; }

extern "C" int pss_regex_info(const pss_regex *rx, pss_regex_dfa *info)
{
    return guarded([&]() -> int {
        if (!rx || !info) {
            set_error("pss_regex_info: bad arguments");
            return PSS_EINVAL;
        }
        const RegexDfa &d = rx->dfa;
        *info = pss_regex_dfa{d.nstates, d.ncls, d.table_bytes(), d.anchors, d.start, d.first_accept, d.sink};
        return PSS_OK;
    });
}

extern "C" int pss_regex_literals(const pss_regex *rx, uint8_t *out, uint64_t cap, uint64_t *offsets, uint32_t *count)
{
    return guarded([&]() -> int {
        if (!rx || !offsets || !count || (cap && !out)) {
            set_error("pss_regex_literals: bad arguments");
            return PSS_EINVAL;
        }
        uint64_t total = 0;
        for (const std::string &lit : rx->dfa.literals) total += lit.size();
        if (!out) {                                  // the sizes alone: what the buffer of the next call has to hold
            uint32_t k = 0;
            offsets[0] = 0;
            for (const std::string &lit : rx->dfa.literals) { offsets[k + 1] = offsets[k] + lit.size(); ++k; }
            *count = k;
            return PSS_OK;
        }
        if (total > cap) {
            set_error("pss_regex_literals: the literals have %llu bytes, the buffer %llu", (unsigned long long)total, (unsigned long long)cap);
            return PSS_EINVAL;
        }
        uint64_t at = 0;
        uint32_t k = 0;
        offsets[0] = 0;
        for (const std::string &lit : rx->dfa.literals) {
            memcpy(out + at, lit.data(), lit.size());
            at += lit.size();
            offsets[++k] = at;
        }
        *count = k;
        return PSS_OK;
    });
}

extern "C" int pss_regex_match(const pss_regex *rx, const uint8_t *bytes, uint64_t len)
{
    return guarded([&]() -> int {
        if (!rx || (len && !bytes)) {
            set_error("pss_regex_match: bad arguments");
            return PSS_EINVAL;
        }
        return regex_match(rx->dfa, bytes, len) ? 1 : 0;
    });
}

extern "C" int pss_reader_search_regex_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                             pss_result **out)
{
    return guarded([&]() -> int { return regex_batch(r, "pss_reader_search_regex_batch", pbytes, poffsets, np, flags, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_regex_ids_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                                 pss_result **out)
{
    return guarded([&]() -> int { return regex_batch(r, "pss_reader_search_regex_ids_batch", pbytes, poffsets, np, flags, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_regex_batch(pss_reader *r, const uint8_t *pbytes, const uint64_t *poffsets, uint32_t np, uint32_t flags,
                                            uint64_t *counts)
{
    return guarded([&]() -> int { return regex_batch(r, "pss_reader_count_regex_batch", pbytes, poffsets, np, flags, SEARCH_COUNTS, nullptr, counts); });
}

// ---- case-insensitive search: group -> terms -> the spellings of a seed (fold_impl.h) --------------

namespace {

// The three plain case-insensitive calls: their own argument checks, then every pattern as a group of one include term.
// The reader is looked at last, as for the all-terms calls: a malformed batch is reported as such with or without one.
int icase_plain(pss_reader *r, const char *who, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, SearchMode mode,
                pss_result **out, uint64_t *counts)
{
    if (!out_ok_by_mode(mode, nq, out, counts) || (nq && (!qbytes || !qoffsets))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    PSS_TRY(pattern_args(who, qoffsets, nq, [](uint32_t, uint64_t) { return true; }));
    SeededGroups b;
    PSS_TRY(icase_expand(who, "pattern", qbytes, qoffsets, nq, &b));
    if (!r) {
        set_error("%s: bad arguments (no reader)", who);
        return PSS_EINVAL;
    }
    b.one_term_each(nq);
    return answer_by_mode(r, b.request(nq, b.one_each.data(), nq, b.no_exclude.data(), nullptr, mode), out, counts);
}

}  // namespace

extern "C" int pss_icase_variants(const uint8_t *pat, uint64_t len, int32_t letters, uint8_t *out, uint64_t cap, uint32_t *seed_off,
                                  uint32_t *seed_len, uint32_t *count)
{
    return guarded([&]() -> int {
        if (!pat || !len) {
            set_error("pss_icase_variants: the pattern is empty (every entry contains the empty pattern)");
            return PSS_EINVAL;
        }
        if (letters > 6 || !seed_off || !seed_len || !count) {
            set_error("pss_icase_variants: bad arguments (letters = %d: 1 .. 6, or <= 0 for PSS_ICASE_SEED_LETTERS)", (int)letters);
            return PSS_EINVAL;
        }
        uint64_t so = 0, sl = 0;
        const uint32_t f = fold_seed(pat, len, icase_letters(letters), &so, &sl);
        if (so > 0xffffffffull || sl > 0xffffffffull) {
            set_error("pss_icase_variants: a pattern of %llu bytes", (unsigned long long)len);
            return PSS_EINVAL;
        }
        *seed_off = (uint32_t)so;
        *seed_len = (uint32_t)sl;
        *count = 1u << f;
        if (!out) return PSS_OK;            // (the sizes alone)
        if (cap < (sl << f)) {
            set_error("pss_icase_variants: %u variants of %llu bytes need more than the %llu bytes of out", 1u << f, (unsigned long long)sl,
                      (unsigned long long)cap);
            return PSS_EINVAL;
        }
        fold_spellings(pat + so, sl, f, out);
        return PSS_OK;
    });
}

extern "C" int pss_reader_search_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, pss_result **out)
{
    return guarded([&]() -> int { return icase_plain(r, "pss_reader_search_icase_batch", qbytes, qoffsets, nq, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_icase_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                 pss_result **out)
{
    return guarded([&]() -> int { return icase_plain(r, "pss_reader_search_icase_ids_batch", qbytes, qoffsets, nq, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, uint64_t *counts)
{
    return guarded([&]() -> int { return icase_plain(r, "pss_reader_count_icase_batch", qbytes, qoffsets, nq, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_reader_search_terms_icase_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, pss_result **out)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_search_terms_icase_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, true, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_terms_icase_ids_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, pss_result **out)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_search_terms_icase_ids_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, true, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_terms_icase_batch(pss_reader *r, const uint8_t *tbytes, const uint64_t *toffsets, uint32_t nterms, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *exclude, uint64_t *counts)
{
    return guarded([&]() -> int { return terms_batch(r, "pss_reader_count_terms_icase_batch", tbytes, toffsets, nterms, group_offsets, ngroups, exclude, true, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_reader_search_seq_icase_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_search_seq_icase_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, true, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_seq_icase_ids_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, pss_result **out)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_search_seq_icase_ids_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, true, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_seq_icase_batch(pss_reader *r, const uint8_t *sbytes, const uint64_t *soffsets, uint32_t nsegs, const uint64_t *group_offsets,
        uint32_t ngroups, const uint8_t *anchors, uint64_t *counts)
{
    return guarded([&]() -> int { return seq_batch(r, "pss_reader_count_seq_icase_batch", sbytes, soffsets, nsegs, group_offsets, ngroups, anchors, true, SEARCH_COUNTS, nullptr, counts); });
}

// ---- search within k mismatches or k edits: pattern -> pattern -> its k + 1 pieces (near_impl.h; -----
// ---- edit_impl.h, 4.17) ---------------------------------------------------------------------------------------------

namespace {

constexpr uint32_t kNearMaxBudget = 3;

// Under fold a piece is looked up as a case-insensitive term is: through the spellings of its seed.  A term keeps at most
// 64 queries, the bound seed_union_kernel and the hit walk were written for, so the seed of a piece of a pattern with budget
// k has at most kNearFoldCap[k] letters: the largest f with (k + 1) 2^f <= 64.
constexpr uint8_t kNearFoldCap[kNearMaxBudget + 1] = {6, 5, 4, 4};

// The seeds of pat[0, len) with budget k < len under fold, piece by piece: emit(piece j, the seed's position inside the
// PATTERN, its length, its letters).  `letters` is the configured limit (1 .. 6), which the cap of k bounds.
template <typename Emit>
void near_fold_seeds(const uint8_t *pat, uint64_t len, uint32_t k, uint32_t letters, Emit emit)
{
    uint64_t off[kNearMaxBudget + 2];
    near_pieces(len, k, off);
    const uint32_t f = std::min<uint32_t>(letters, kNearFoldCap[k]);
    for (uint32_t j = 0; j <= k; ++j) {
        uint64_t so = 0, sl = 0;
        const uint32_t nl = fold_seed(pat + off[j], off[j + 1] - off[j], f, &so, &sl);
        emit(j, off[j] + so, sl, nl);
    }
}

// A batch that near_plain has judged, under ASCII case folding: the terms are the patterns folded to
// lower case, and a pattern's seed queries are, piece by piece, the spellings of the piece's seed in ascending order, each
// at the seed's position inside the pattern.  The queries of one term are piece-major; spellings of one piece have disjoint
// intervals, but pieces may overlap, nest or repeat, so the batch hands seed_union_kernel the overflow flag as every near
// batch does.  At k = 0 the queries are exactly those of icase_expand.
int near_fold_plain(pss_reader *r, const char *who, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                    bool edits, SearchMode mode, pss_result **out, uint64_t *counts)
{
    const uint32_t letters = icase_letters(0);
    const uint64_t total = nq ? qoffsets[nq] : 0;
    SeededGroups b;
    b.fbytes.resize(total + 1);
    for (uint64_t i = 0; i < total; ++i) b.fbytes[i] = (uint8_t)((uint8_t)(qbytes[i] - 'A') < 26 ? qbytes[i] | 0x20 : qbytes[i]);
    b.voff.assign(1, 0);
    b.soff.assign(1, 0);
    b.soff.reserve((size_t)nq + 1);
    for (uint32_t q = 0; q < nq; ++q) {
        const uint8_t *pat = qbytes + qoffsets[q];
        uint64_t nqueries = b.soff.back();
        near_fold_seeds(pat, qoffsets[q + 1] - qoffsets[q], k[q], letters, [&](uint32_t, uint64_t at, uint64_t sl, uint32_t nl) {
            const size_t o = b.vbytes.size();
            b.vbytes.resize(o + (size_t)(sl << nl));
            fold_spellings(pat + at, sl, nl, b.vbytes.data() + o);
            for (uint32_t v = 0; v < (1u << nl); ++v) {
                b.voff.push_back(b.voff.back() + sl);
                b.pos.push_back((uint32_t)at);
            }
            nqueries += 1ull << nl;
        });
        if (nqueries > 0xffffffffull) {
            set_error("%s: the patterns expand to more than the 2^32 - 1 seed queries a batch takes (at pattern %u)", who, q);
            return PSS_EINVAL;
        }
        b.soff.push_back(nqueries);
    }
    b.vbytes.push_back(0);                   // (data() of an empty vector may be null)
    b.pos.push_back(0);
    b.one_term_each(nq);
    static const uint8_t no_budget = 0;
    static const uint64_t no_offset = 0;
    SearchRequest rq = b.request(nq, b.one_each.data(), nq, b.no_exclude.data(), nullptr, mode);
    rq.term_offsets = nq ? qoffsets : &no_offset;
    rq.near_budget = nq ? k : &no_budget;
    rq.near_edits = edits;
    rq.near_fold = true;
    return answer_by_mode(r, rq, out, counts);
}

// The three calls within k mismatches and the three within k edits (`edits`: what the budget counts, and the one
// difference of the request), and the three of either under fold (`fold`: near_fold_plain takes the judged batch): their own argument checks, then every pattern cut into its pieces -- the seed queries of a
// group of one include term.  The patterns' own bytes and offsets are the caller's.  As for icase_plain, a malformed batch
// is reported as such with or without a reader: the reader is looked at last.
int near_plain(pss_reader *r, const char *who, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
               bool edits, bool fold, SearchMode mode, pss_result **out, uint64_t *counts)
{
    const char *unit = edits ? "edits" : "mismatches";
    if (!out_ok_by_mode(mode, nq, out, counts) || (nq && (!qbytes || !qoffsets || !k))) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    uint64_t npieces = 0;
    PSS_TRY(pattern_args(who, qoffsets, nq, [&](uint32_t q, uint64_t len) {
        if (k[q] > kNearMaxBudget) {
            set_error("%s: pattern %u has a budget of %u %s: 0 .. %u", who, q, (unsigned)k[q], unit, kNearMaxBudget);
            return false;
        }
        if (len <= k[q]) {
            set_error("%s: pattern %u has %llu bytes and a budget of %u %s: %s "
                      "(a pattern is longer than its budget)", who, q, (unsigned long long)len, (unsigned)k[q], unit,
                      edits ? "deleting all of it matches every entry" : "every window of its length matches it");
            return false;
        }
        npieces += (uint64_t)k[q] + 1;
        return true;
    }));
    if (npieces > 0xffffffffull) {
        set_error("%s: the patterns are cut into more than the 2^32 - 1 pieces a batch takes", who);
        return PSS_EINVAL;
    }
    if (!r) {
        set_error("%s: bad arguments (no reader)", who);
        return PSS_EINVAL;
    }
    if (fold) return near_fold_plain(r, who, qbytes, qoffsets, nq, k, edits, mode, out, counts);
    SeededGroups b;
    b.voff.reserve(npieces + 1);
    b.pos.reserve(npieces + 1);
    b.voff.assign(1, 0);
    b.soff.assign(1, 0);
    b.soff.reserve((size_t)nq + 1);
    for (uint32_t q = 0; q < nq; ++q) {
        uint64_t off[kNearMaxBudget + 2];
        near_pieces(qoffsets[q + 1] - qoffsets[q], k[q], off);
        for (uint32_t j = 0; j <= k[q]; ++j) {
            b.pos.push_back((uint32_t)off[j]);
            b.voff.push_back(b.voff.back() + (off[j + 1] - off[j]));
        }
        b.soff.push_back(b.soff.back() + k[q] + 1);
    }
    // (the pieces of a pattern partition it, so back to back they are the patterns' bytes again)
    b.vbytes.assign(qbytes, qbytes + (nq ? qoffsets[nq] : 0));
    b.vbytes.push_back(0);                   // (data() of an empty vector may be null)
    b.pos.push_back(0);
    b.one_term_each(nq);
    static const uint8_t no_budget = 0;
    static const uint64_t no_offset = 0;
    SearchRequest rq = b.request(nq, b.one_each.data(), nq, b.no_exclude.data(), nullptr, mode);
    rq.term_bytes = b.vbytes.data();
    rq.term_offsets = nq ? qoffsets : &no_offset;
    rq.near_budget = nq ? k : &no_budget;
    rq.near_edits = edits;
    return answer_by_mode(r, rq, out, counts);
}

}  // namespace

extern "C" int pss_near_pieces(const uint8_t *pat, uint64_t len, uint32_t k, uint32_t *offsets, uint32_t *lengths, uint32_t *count)
{
    return guarded([&]() -> int {
        if (!pat || !len) {
            set_error("pss_near_pieces: the pattern is empty (every entry contains the empty pattern)");
            return PSS_EINVAL;
        }
        if (k > kNearMaxBudget) {
            set_error("pss_near_pieces: a budget of %u mismatches: 0 .. %u", k, kNearMaxBudget);
            return PSS_EINVAL;
        }
        if (len <= k) {
            set_error("pss_near_pieces: a pattern of %llu bytes and a budget of %u mismatches: every window of its length matches it "
                      "(a pattern is longer than its budget)", (unsigned long long)len, k);
            return PSS_EINVAL;
        }
        if (len > 0xffffffffull || !offsets || !lengths || !count) {
            set_error("pss_near_pieces: bad arguments (a pattern of %llu bytes)", (unsigned long long)len);
            return PSS_EINVAL;
        }
        uint64_t off[kNearMaxBudget + 2];
        near_pieces(len, k, off);
        for (uint32_t j = 0; j <= k; ++j) {
            offsets[j] = (uint32_t)off[j];
            lengths[j] = (uint32_t)(off[j + 1] - off[j]);
        }
        *count = k + 1;
        return PSS_OK;
    });
}

extern "C" int pss_reader_search_near_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                            pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_near_batch", qbytes, qoffsets, nq, k, false, false, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_near_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                                pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_near_ids_batch", qbytes, qoffsets, nq, k, false, false, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_near_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                           uint64_t *counts)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_count_near_batch", qbytes, qoffsets, nq, k, false, false, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_reader_search_edit_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                            pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_edit_batch", qbytes, qoffsets, nq, k, true, false, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_edit_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                                pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_edit_ids_batch", qbytes, qoffsets, nq, k, true, false, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_edit_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq, const uint8_t *k,
                                           uint64_t *counts)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_count_edit_batch", qbytes, qoffsets, nq, k, true, false, SEARCH_COUNTS, nullptr, counts); });
}

/* ---- the same two searches under ASCII case folding ---- */

extern "C" int pss_reader_search_near_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                  const uint8_t *k, int edits, pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_near_icase_batch", qbytes, qoffsets, nq, k, edits != 0, true, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_near_icase_ids_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                      const uint8_t *k, int edits, pss_result **out)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_search_near_icase_ids_batch", qbytes, qoffsets, nq, k, edits != 0, true, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_near_icase_batch(pss_reader *r, const uint8_t *qbytes, const uint64_t *qoffsets, uint32_t nq,
                                                 const uint8_t *k, int edits, uint64_t *counts)
{
    return guarded([&]() -> int { return near_plain(r, "pss_reader_count_near_icase_batch", qbytes, qoffsets, nq, k, edits != 0, true, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_near_seeds(const uint8_t *pat, uint64_t len, uint32_t k, int32_t letters, uint8_t *out, uint64_t cap, uint32_t *piece,
                              uint32_t *pos, uint32_t *lengths, uint32_t *count)
{
    return guarded([&]() -> int {
        if (!pat || !len) {
            set_error("pss_near_seeds: the pattern is empty (every entry contains the empty pattern)");
            return PSS_EINVAL;
        }
        if (k > kNearMaxBudget) {
            set_error("pss_near_seeds: a budget of %u: 0 .. %u", k, kNearMaxBudget);
            return PSS_EINVAL;
        }
        if (len <= k) {
            set_error("pss_near_seeds: a pattern of %llu bytes and a budget of %u (a pattern is longer than its budget)",
                      (unsigned long long)len, k);
            return PSS_EINVAL;
        }
        if (letters > 6 || len > 0xffffffffull || !piece || !pos || !lengths || !count) {
            set_error("pss_near_seeds: bad arguments (letters = %d: 1 .. 6, or <= 0 for PSS_ICASE_SEED_LETTERS; a pattern of %llu bytes)",
                      (int)letters, (unsigned long long)len);
            return PSS_EINVAL;
        }
        uint32_t n = 0;
        uint64_t bytes = 0;
        bool fits = true;
        near_fold_seeds(pat, len, k, icase_letters(letters), [&](uint32_t j, uint64_t at, uint64_t sl, uint32_t nl) {
            fits = fits && (!out || bytes + (sl << nl) <= cap);
            if (out && fits) fold_spellings(pat + at, sl, nl, out + bytes);
            for (uint32_t v = 0; v < (1u << nl); ++v, ++n) {      // (at most 64 in all: the cap)
                piece[n] = j;
                pos[n] = (uint32_t)at;
                lengths[n] = (uint32_t)sl;
            }
            bytes += sl << nl;
        });
        *count = n;
        if (!fits) {
            set_error("pss_near_seeds: %u queries need %llu bytes, more than the %llu bytes of out", n, (unsigned long long)bytes,
                      (unsigned long long)cap);
            return PSS_EINVAL;
        }
        return PSS_OK;
    });
}

// ---- any-of search: set -> its normalised alternatives as one term -> the alternatives, or the spellings of their seeds ----
// ---- (any_terms.h, any_impl.h) ---------------------------------------------------------------------------

namespace {

// Set g = alternatives first .. last of the batch, judged and normalised (any_terms.h): no set is empty, no alternative is
// empty or has more than 2^32 - 1 bytes, and at most 64 alternatives are left, 32 under fold.
int any_set(const char *who, uint64_t g, const uint8_t *abytes, const uint64_t *aoffsets, uint64_t first, uint64_t last, bool fold, AnySet *set)
{
    if (first == last) {
        set_error("%s: set %llu: no alternative (a set without one matches nothing: leave it out)", who, (unsigned long long)g);
        return PSS_EINVAL;
    }
    for (uint64_t a = first; a < last; ++a) {
        const uint64_t len = aoffsets[a + 1] - aoffsets[a];
        if (len == 0 || len > 0xffffffffull) {
            set_error(len ? "%s: set %llu: alternative %llu has more than 2^32 - 1 bytes (a chunk has fewer)"
                          : "%s: set %llu: alternative %llu is empty (every entry contains it)",
                      who, (unsigned long long)g, (unsigned long long)(a - first));
            return PSS_EINVAL;
        }
    }
    *set = any_normalise(abytes, aoffsets, first, last, fold);
    const uint32_t cap = fold ? ANY_MAX_ALTS_FOLD : ANY_MAX_ALTS;
    if (set->alts.size() > cap) {
        set_error("%s: set %llu: %llu alternatives after normalisation, more than the %u a set takes%s", who, (unsigned long long)g,
                  (unsigned long long)set->alts.size(), cap, fold ? " under PSS_ANY_ICASE" : "");
        return PSS_EINVAL;
    }
    return PSS_OK;
}

// The seed of one alternative of a normalised set of n under fold (letters: the configured limit).
uint32_t any_seed(const std::string &alt, uint32_t n, uint32_t letters, uint64_t *so, uint64_t *sl)
{
    return fold_seed(reinterpret_cast<const uint8_t *>(alt.data()), alt.size(), any_seed_letters(n, letters), so, sl);
}

// The flags and offsets of the any-of calls, in the documented order (the output argument is the caller's to judge first).
int any_args(const char *who, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts, const uint64_t *set_offsets, uint32_t nsets,
             uint32_t flags)
{
    if ((nalts && (!abytes || !aoffsets)) || (nsets && !set_offsets)) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    if (flags & ~PSS_ANY_ICASE) {
        set_error("%s: flags = %u (PSS_ANY_ICASE = 1 or nothing)", who, flags);
        return PSS_EINVAL;
    }
    if (nalts && aoffsets[0] != 0) {
        set_error("%s: the alternative offsets start at %llu, not at 0", who, (unsigned long long)aoffsets[0]);
        return PSS_EINVAL;
    }
    for (uint32_t a = 0; a < nalts; ++a)
        if (aoffsets[a + 1] < aoffsets[a]) {
            set_error("%s: the alternative offsets decrease at alternative %u", who, a);
            return PSS_EINVAL;
        }
    if (nsets && set_offsets[0] != 0) {
        set_error("%s: the set offsets start at %llu, not at 0", who, (unsigned long long)set_offsets[0]);
        return PSS_EINVAL;
    }
    for (uint32_t g = 0; g < nsets; ++g)
        if (set_offsets[g + 1] < set_offsets[g]) {
            set_error("%s: the set offsets decrease at set %u", who, g);
            return PSS_EINVAL;
        }
    if (nsets && set_offsets[nsets] != nalts) {
        set_error("%s: the set offsets end at %llu, not at the %u alternatives", who, (unsigned long long)set_offsets[nsets], nalts);
        return PSS_EINVAL;
    }
    return PSS_OK;
}

// The three any-of calls: their own argument checks, then every set as a group of one include term -- its normalised
// alternatives back to back -- whose seed queries are the alternatives themselves or, under fold, alternative by
// alternative the spellings of its seed.  The reader is looked at last, as for the other seeded calls.
int any_batch(pss_reader *r, const char *who, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts, const uint64_t *set_offsets,
              uint32_t nsets, uint32_t flags, SearchMode mode, pss_result **out, uint64_t *counts)
{
    if (!out_ok_by_mode(mode, nsets, out, counts)) {
        set_error("%s: bad arguments", who);
        return PSS_EINVAL;
    }
    PSS_TRY(any_args(who, abytes, aoffsets, nalts, set_offsets, nsets, flags));
    const bool fold = (flags & PSS_ANY_ICASE) != 0;
    const uint32_t letters = icase_letters(0);
    SeededGroups b;
    std::vector<uint64_t> talts(1, 0), aoff(1, 0);
    std::vector<uint32_t> qalt;
    b.voff.assign(1, 0);
    b.soff.assign(1, 0);
    b.foff.assign(1, 0);
    for (uint32_t g = 0; g < nsets; ++g) {
        AnySet set;
        PSS_TRY(any_set(who, g, abytes, aoffsets, set_offsets[g], set_offsets[g + 1], fold, &set));
        const uint32_t n = (uint32_t)set.alts.size();
        for (const std::string &alt : set.alts) {
            const uint32_t j = (uint32_t)(aoff.size() - 1);
            b.fbytes.insert(b.fbytes.end(), alt.begin(), alt.end());
            aoff.push_back(b.fbytes.size());
            uint64_t so = 0, sl = alt.size();
            const uint32_t nl = fold ? any_seed(alt, n, letters, &so, &sl) : 0;
            const size_t o = b.vbytes.size();
            b.vbytes.resize(o + (size_t)(sl << nl));
            if (fold)
                fold_spellings(reinterpret_cast<const uint8_t *>(alt.data()) + so, sl, nl, b.vbytes.data() + o);
            else
                memcpy(b.vbytes.data() + o, alt.data(), alt.size());
            for (uint32_t v = 0; v < (1u << nl); ++v) {          // (exact: one query, the alternative itself at 0)
                b.voff.push_back(b.voff.back() + sl);
                b.pos.push_back((uint32_t)so);
                qalt.push_back(j);
            }
        }
        if (b.voff.size() - 1 > 0xffffffffull || aoff.size() - 1 > 0xffffffffull) {
            set_error("%s: the sets expand to more than the 2^32 - 1 seed queries a batch takes (at set %u)", who, g);
            return PSS_EINVAL;
        }
        talts.push_back(aoff.size() - 1);
        b.foff.push_back(b.fbytes.size());
        b.soff.push_back(b.voff.size() - 1);
    }
    if (!r) {
        set_error("%s: bad arguments (no reader)", who);
        return PSS_EINVAL;
    }
    b.fbytes.push_back(0);                   // (data() of an empty vector may be null)
    b.vbytes.push_back(0);
    b.pos.push_back(0);
    qalt.push_back(0);
    b.one_term_each(nsets);
    SearchRequest rq = b.request(nsets, b.one_each.data(), nsets, b.no_exclude.data(), nullptr, mode);
    rq.any_term_alts = talts.data();
    rq.any_alt_offsets = aoff.data();
    rq.any_query_alt = qalt.data();
    rq.any_nalts = (uint32_t)(aoff.size() - 1);
    rq.any_fold = fold;
    return answer_by_mode(r, rq, out, counts);
}

}  // namespace

extern "C" int pss_reader_search_any_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                                           const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, pss_result **out)
{
    return guarded([&]() -> int { return any_batch(r, "pss_reader_search_any_batch", abytes, aoffsets, nalts, set_offsets, nsets, flags, SEARCH_FULL, out, nullptr); });
}

extern "C" int pss_reader_search_any_ids_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                                               const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, pss_result **out)
{
    return guarded([&]() -> int { return any_batch(r, "pss_reader_search_any_ids_batch", abytes, aoffsets, nalts, set_offsets, nsets, flags, SEARCH_IDS, out, nullptr); });
}

extern "C" int pss_reader_count_any_batch(pss_reader *r, const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts,
                                          const uint64_t *set_offsets, uint32_t nsets, uint32_t flags, uint64_t *counts)
{
    return guarded([&]() -> int { return any_batch(r, "pss_reader_count_any_batch", abytes, aoffsets, nalts, set_offsets, nsets, flags, SEARCH_COUNTS, nullptr, counts); });
}

extern "C" int pss_any_alternatives(const uint8_t *abytes, const uint64_t *aoffsets, uint32_t nalts, uint32_t flags, int32_t letters,
                                    uint8_t *out, uint64_t cap, uint64_t *offsets, uint32_t *seed_pos, uint32_t *seed_len, uint32_t *count)
{
    return guarded([&]() -> int {
        const char *who = "pss_any_alternatives";
        if (!out || !offsets || !seed_pos || !seed_len || !count || letters > 6) {
            set_error("%s: bad arguments (letters = %d: 1 .. 6, or <= 0 for PSS_ICASE_SEED_LETTERS)", who, (int)letters);
            return PSS_EINVAL;
        }
        const uint64_t one_set[2] = {0, nalts};
        PSS_TRY(any_args(who, abytes, aoffsets, nalts, one_set, 1, flags));
        const bool fold = (flags & PSS_ANY_ICASE) != 0;
        AnySet set;
        PSS_TRY(any_set(who, 0, abytes, aoffsets, 0, nalts, fold, &set));
        uint64_t total = 0;
        for (const std::string &alt : set.alts) total += alt.size();
        if (total > cap) {
            set_error("%s: the alternatives need %llu bytes, more than the %llu bytes of out", who, (unsigned long long)total,
                      (unsigned long long)cap);
            return PSS_EINVAL;
        }
        const uint32_t n = (uint32_t)set.alts.size();
        offsets[0] = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const std::string &alt = set.alts[j];
            memcpy(out + offsets[j], alt.data(), alt.size());
            offsets[j + 1] = offsets[j] + alt.size();
            uint64_t so = 0, sl = alt.size();
            if (fold) any_seed(alt, n, icase_letters(letters), &so, &sl);
            seed_pos[j] = (uint32_t)so;
            seed_len[j] = (uint32_t)sl;
        }
        *count = n;
        return PSS_OK;
    });
}

namespace {

// ids[0 .. n) of ONE single-device reader as (resident chunk, line) pairs, validated on the host (the reader knows every
// chunk's entry count once the line tables exist).
int reader_resolve_ids(pss_reader *x, const uint64_t *ids, uint64_t n, std::vector<uint32_t> &chunk_of, std::vector<uint32_t> &line_of)
{
    chunk_of.resize(n);
    line_of.resize(n);
    size_t at = 0;                                   // (consecutive ids mostly name the same chunk)
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t c = ids[i] >> 32;
        const uint32_t line = (uint32_t)ids[i];
        if (at >= x->file_index.size() || x->file_index[at] != c) {
            for (at = 0; at < x->file_index.size() && x->file_index[at] != c; ++at) {}
        }
        if (at == x->file_index.size()) {
            set_error("entry id %#llx: this reader does not hold chunk %llu", (unsigned long long)ids[i], (unsigned long long)c);
            return PSS_EINVAL;
        }
        if (line >= x->mem[at].entries) {
            set_error("entry id %#llx: chunk %llu has %u entries", (unsigned long long)ids[i], (unsigned long long)c, x->mem[at].entries);
            return PSS_EINVAL;
        }
        chunk_of[i] = (uint32_t)at;
        line_of[i] = line;
    }
    return PSS_OK;
}

// ids[0 .. n) of ONE single-device reader: validation on the host, select + copy on the device.
int reader_entries_single(pss_reader *x, const uint64_t *ids, uint64_t n, HostResult *res)
{
    std::lock_guard<std::recursive_mutex> lk(x->ctx->mu);
    PSS_HIP(hipSetDevice(x->device));
    PSS_TRY(reader_sync_descs(x));
    PSS_TRY(reader_ensure_lines(x));
    std::vector<uint32_t> chunk_of, line_of;
    PSS_TRY(reader_resolve_ids(x, ids, n, chunk_of, line_of));
    return entries_by_id_device(x->ctx, x->d_descs, x->d_lines, chunk_of.data(), line_of.data(), n, res);
}

// The judged patterns of a span batch as the device reads them: folded to lower case under ICASE, kSpanPatPad zero bytes
// behind them, and per pattern whether it holds a newline (then all its rows are no match).
struct SpanPatterns {
    std::vector<uint8_t> bytes, has_nl;
    const uint64_t *off;
    const uint8_t *k;
    uint32_t nq;
    bool edits, fold;
};

// Rows of ONE single-device reader: ids[i] against pattern pat_of[i]; out[i] answers ids[i].
int reader_spans_single(pss_reader *x, const uint64_t *ids, const uint32_t *pat_of, uint64_t n, const SpanPatterns &P, pss_span *out)
{
    std::lock_guard<std::recursive_mutex> lk(x->ctx->mu);
    PSS_HIP(hipSetDevice(x->device));
    PSS_TRY(reader_sync_descs(x));
    PSS_TRY(reader_ensure_lines(x));
    std::vector<uint32_t> chunk_of, line_of;
    PSS_TRY(reader_resolve_ids(x, ids, n, chunk_of, line_of));
    static_assert(sizeof(pss_span) == 12, "three int32 a row");
    return match_spans_device(x->ctx, x->d_descs, x->d_lines, chunk_of.data(), line_of.data(), pat_of, n, P.bytes.data(), P.off, P.nq, P.k,
                              P.has_nl.data(), P.edits, P.fold, reinterpret_cast<int32_t *>(out));
}

}  // namespace

extern "C" int pss_reader_entries_by_id(pss_reader *r, const uint64_t *ids, uint64_t n, pss_result **out)
{
    return guarded([&]() -> int {
        if (!r || !out || (n && !ids)) {
            set_error("pss_reader_entries_by_id: bad arguments");
            return PSS_EINVAL;
        }
        pss_result *res = new pss_result();
        struct Drop {
            pss_result *p;
            ~Drop() { if (p) pss_result_free(p); }
        } drop{res};
        if (r->parts.empty()) {
            PSS_TRY(reader_entries_single(r, ids, n, &res->r));
        } else {
            // every part fetches the entries of its chunks (one part after the other: a fetch is two small kernels and a
            // copy), then the texts are put back in the order asked
            std::lock_guard<std::mutex> batch(r->multi_mu);
            const size_t G = r->parts.size();
            std::vector<std::vector<uint64_t>> sub(G);
            std::vector<uint32_t> part_of(n);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t c = ids[i] >> 32;
                size_t g = 0;
                for (; g < G; ++g) {
                    const std::vector<uint64_t> &fi = r->parts[g]->reader->file_index;
                    if (std::find(fi.begin(), fi.end(), c) != fi.end()) break;
                }
                if (g == G) {
                    set_error("entry id %#llx: this reader does not hold chunk %llu", (unsigned long long)ids[i], (unsigned long long)c);
                    return PSS_EINVAL;
                }
                part_of[i] = (uint32_t)g;
                sub[g].push_back(ids[i]);
            }
            std::vector<HostResult> pr(G);
            struct Release {
                std::vector<HostResult> &v;
                ~Release() { for (auto &x : v) x.release(); }
            } release{pr};
            uint64_t B = 0;
            for (size_t g = 0; g < G; ++g) {
                if (sub[g].empty()) continue;
                PSS_TRY(reader_entries_single(r->parts[g]->reader, sub[g].data(), sub[g].size(), &pr[g]));
                B += pr[g].n_bytes;
            }
            HostResult &o = res->r;
            o.nq = n;
            o.qcount = static_cast<uint64_t *>(malloc((n ? n : 1) * sizeof(uint64_t)));
            if (!o.qcount) return PSS_ENOMEM;
            PSS_TRY(alloc_host_result(&o, n, B, !search_knobs().no_pinned_results));
            std::vector<uint64_t> cursor(G, 0);
            uint64_t b = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const HostResult &p = pr[part_of[i]];
                const uint64_t e = cursor[part_of[i]]++;
                const uint64_t len = p.offsets[e + 1] - p.offsets[e];
                o.qcount[i] = 1;
                o.offsets[i] = b;
                if (len) memcpy(o.bytes + b, p.bytes + p.offsets[e], (size_t)len);
                b += len;
            }
            o.offsets[n] = b;
            o.n_entries = n;
            o.n_bytes = b;
        }
        drop.p = nullptr;
        *out = res;
        return PSS_OK;
    });
}

extern "C" int pss_reader_match_spans(pss_reader *r, const uint64_t *ids, const uint64_t *id_offsets, const uint8_t *qbytes,
                                      const uint64_t *qoffsets, uint32_t nq, const uint8_t *k, uint32_t flags, pss_span *out)
{
    return guarded([&]() -> int {
        const char *who = "pss_reader_match_spans";
        if (nq && (!id_offsets || !qbytes || !qoffsets || !k)) {
            set_error("%s: bad arguments", who);
            return PSS_EINVAL;
        }
        const bool edits = (flags & PSS_SPAN_EDITS) != 0, fold = (flags & PSS_SPAN_ICASE) != 0;
        const char *unit = edits ? "edits" : "mismatches";
        PSS_TRY(pattern_args(who, qoffsets, nq, [&](uint32_t q, uint64_t len) {
            if (k[q] > kNearMaxBudget) {
                set_error("%s: pattern %u has a budget of %u %s: 0 .. %u", who, q, (unsigned)k[q], unit, kNearMaxBudget);
                return false;
            }
            if (len <= k[q]) {
                set_error("%s: pattern %u has %llu bytes and a budget of %u %s (a pattern is longer than its budget)", who, q,
                          (unsigned long long)len, (unsigned)k[q], unit);
                return false;
            }
            return true;
        }));
        if (flags & ~(PSS_SPAN_EDITS | PSS_SPAN_ICASE)) {
            set_error("%s: unknown flag bits %#x (PSS_SPAN_EDITS | PSS_SPAN_ICASE)", who, flags);
            return PSS_EINVAL;
        }
        if (nq && id_offsets[0] != 0) {
            set_error("%s: the id offsets start at %llu, not at 0", who, (unsigned long long)id_offsets[0]);
            return PSS_EINVAL;
        }
        for (uint32_t q = 0; q < nq; ++q)
            if (id_offsets[q + 1] < id_offsets[q]) {
                set_error("%s: the id offsets decrease at pattern %u", who, q);
                return PSS_EINVAL;
            }
        const uint64_t n = nq ? id_offsets[nq] : 0;
        if (n && (!ids || !out)) {
            set_error("%s: bad arguments (%llu rows without ids or room for the answer)", who, (unsigned long long)n);
            return PSS_EINVAL;
        }
        if (!r) {
            set_error("%s: bad arguments (no reader)", who);
            return PSS_EINVAL;
        }
        if (n == 0) return PSS_OK;
        SpanPatterns P;
        const uint64_t total = qoffsets[nq];
        P.bytes.assign((size_t)total + kSpanPatPad, 0);
        for (uint64_t i = 0; i < total; ++i)
            P.bytes[i] = (uint8_t)(fold && (uint8_t)(qbytes[i] - 'A') < 26 ? qbytes[i] | 0x20 : qbytes[i]);
        P.has_nl.resize(nq);
        for (uint32_t q = 0; q < nq; ++q) P.has_nl[q] = memchr(qbytes + qoffsets[q], '\n', (size_t)(qoffsets[q + 1] - qoffsets[q])) ? 1 : 0;
        P.off = qoffsets;
        P.k = k;
        P.nq = nq;
        P.edits = edits;
        P.fold = fold;
        std::vector<uint32_t> pat_of(n);
        for (uint32_t q = 0; q < nq; ++q)
            for (uint64_t i = id_offsets[q]; i < id_offsets[q + 1]; ++i) pat_of[i] = q;
        if (r->parts.empty()) return reader_spans_single(r, ids, pat_of.data(), n, P, out);
        // every part answers the rows of its chunks (one part after the other), then the answers go back in the order asked
        std::lock_guard<std::mutex> batch(r->multi_mu);
        const size_t G = r->parts.size();
        std::vector<std::vector<uint64_t>> sub(G), row_of(G);
        std::vector<std::vector<uint32_t>> sub_pat(G);
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t c = ids[i] >> 32;
            size_t g = 0;
            for (; g < G; ++g) {
                const std::vector<uint64_t> &fi = r->parts[g]->reader->file_index;
                if (std::find(fi.begin(), fi.end(), c) != fi.end()) break;
            }
            if (g == G) {
                set_error("entry id %#llx: this reader does not hold chunk %llu", (unsigned long long)ids[i], (unsigned long long)c);
                return PSS_EINVAL;
            }
            sub[g].push_back(ids[i]);
            sub_pat[g].push_back(pat_of[i]);
            row_of[g].push_back(i);
        }
        // (into a buffer of its own first: an id that a part refuses must leave `out` untouched)
        std::vector<pss_span> all(n), part;
        for (size_t g = 0; g < G; ++g) {
            if (sub[g].empty()) continue;
            part.resize(sub[g].size());
            PSS_TRY(reader_spans_single(r->parts[g]->reader, sub[g].data(), sub_pat[g].data(), sub[g].size(), P, part.data()));
            for (size_t j = 0; j < part.size(); ++j) all[row_of[g][j]] = part[j];
        }
        memcpy(out, all.data(), (size_t)n * sizeof(pss_span));
        return PSS_OK;
    });
}

extern "C" int pss_reader_chunk_entries(pss_reader *r, uint64_t *chunk_index, uint64_t *entries, uint64_t cap, uint64_t *num)
{
    return guarded([&]() -> int {
        if (!r) return PSS_EINVAL;
        std::vector<std::pair<uint64_t, uint64_t>> all;
        auto add = [&](pss_reader *x) -> int {
            if (!x->ctx) return PSS_OK;
            std::lock_guard<std::recursive_mutex> lk(x->ctx->mu);
            PSS_HIP(hipSetDevice(x->device));
            PSS_TRY(reader_sync_descs(x));
            PSS_TRY(reader_ensure_lines(x));
            for (size_t c = 0; c < x->chunks.size(); ++c) all.emplace_back(x->file_index[c], (uint64_t)x->mem[c].entries);
            return PSS_OK;
        };
        if (r->parts.empty()) PSS_TRY(add(r));
        for (pss_reader::Part *p : r->parts) PSS_TRY(add(p->reader));
        std::sort(all.begin(), all.end());
        for (size_t i = 0; i < all.size() && i < cap; ++i) {
            if (chunk_index) chunk_index[i] = all[i].first;
            if (entries) entries[i] = all[i].second;
        }
        if (num) *num = all.size();
        return PSS_OK;
    });
}

// Host merge of per-rank packed results into one, query-major (reference: every chunk task extends one
// Mutex<Vec>, src/lib.rs:280-284; here the ranks' results are concatenated per query, rank-major inside
// a query).  One memcpy per (query, rank) segment -- a rank's entries of one query are contiguous.
extern "C" int pss_merge_packed(uint32_t world, uint64_t nq, const uint64_t *const *counts, const uint64_t *const *offsets,
                                const uint8_t *const *bytes, const uint64_t *num_entries, const uint64_t *num_bytes,
                                uint64_t *out_counts, uint64_t *out_offsets, uint8_t *out_bytes)
{
    return guarded([&]() -> int {
        if (!world || !counts || !offsets || !bytes || !num_entries || !num_bytes || !out_counts || !out_offsets) {
            set_error("pss_merge_packed: bad arguments");
            return PSS_EINVAL;
        }
        std::vector<uint64_t> cursor(world, 0);      // next entry of each rank
        uint64_t e_out = 0, b_out = 0;
        for (uint64_t q = 0; q < nq; ++q) {
            uint64_t tot = 0;
            for (uint32_t r = 0; r < world; ++r) {
                const uint64_t k = counts[r][q];
                if (!k) continue;
                const uint64_t e0 = cursor[r], e1 = e0 + k;
                if (e1 > num_entries[r]) {
                    set_error("pss_merge_packed: rank %u counts exceed its %llu entries", r, (unsigned long long)num_entries[r]);
                    return PSS_EINVAL;
                }
                const uint64_t b0 = offsets[r][e0];
                const uint64_t b1 = e1 < num_entries[r] ? offsets[r][e1] : num_bytes[r];
                if (b0 > b1 || b1 > num_bytes[r]) {      // offsets must grow and stay inside the rank's bytes
                    set_error("pss_merge_packed: rank %u offsets are not monotonic or exceed its %llu bytes", r,
                              (unsigned long long)num_bytes[r]);
                    return PSS_EINVAL;
                }
                for (uint64_t e = e0; e < e1; ++e) {
                    if (offsets[r][e] < b0 || offsets[r][e] > b1) {
                        set_error("pss_merge_packed: rank %u offsets are not monotonic", r);
                        return PSS_EINVAL;
                    }
                    out_offsets[e_out++] = b_out + (offsets[r][e] - b0);
                }
                if (b1 > b0) memcpy(out_bytes + b_out, bytes[r] + b0, (size_t)(b1 - b0));
                b_out += b1 - b0;
                cursor[r] = e1;
                tot += k;
            }
            out_counts[q] = tot;
        }
        out_offsets[e_out] = b_out;
        return PSS_OK;
    });
}

extern "C" int pss_merge_packed_device(int32_t device, uint32_t world, uint64_t nq, const void *const *d_counts,
                                       const void *const *d_starts, const void *const *d_bytes, const uint64_t *num_entries,
                                       const uint64_t *num_bytes, void *d_out_counts, void *d_out_offsets, void *d_out_bytes)
{
    return guarded([&]() -> int {
        if (!world || !d_counts || !d_starts || !d_bytes || !num_entries || !num_bytes || !d_out_counts || !d_out_offsets) {
            set_error("pss_merge_packed_device: bad arguments");
            return PSS_EINVAL;
        }
        DeviceCtx *ctx;
        PSS_TRY(get_ctx(device, &ctx));
        std::lock_guard<std::recursive_mutex> lk(ctx->mu);
        return merge_packed_device(ctx, world, nq, d_counts, d_starts, d_bytes, num_entries, num_bytes, d_out_counts, d_out_offsets,
                                   d_out_bytes);
    });
}
