// kc_api.cpp — the C ABI of include/kc.h except counting (kc_count.cpp), ingest
// (kc_ingest.cpp) and the finish (kc_finish.cpp): the context's lifecycle and
// buffers (kc_ctx.h), records and output, statistics, the file merges, synth,
// queries and set operations.
//
// Replaces PrepareGPU / processKMers / FreeGPU (GPUHandler.cu:397-519) and the
// host aggregation of KMerCounter (KMerCounter.cpp:51-106).
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <memory>
#include <new>

#include "kc_ctx.h"
#include "kc_io.h"

static std::atomic<uint64_t> g_ctx_seq(0);

kc_status fail(kc_ctx* c, kc_status s, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return s;
}

kc_status ensure(kc_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return KC_OK;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        b.release();
    }
    HIPCHK(c, b.alloc(bytes < 256 ? 256 : bytes));
    return KC_OK;
}

// As ensure, but a pooled run buffer that is big enough (best fit) is swapped
// in before anything is allocated: finished runs, merge outputs and fin_packed
// trade the same few large buffers instead of reallocating tens of GB per pass.
kc_status ensure_pooled(kc_ctx* c, DevBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return KC_OK;
    int best = -1;
    for (size_t i = 0; i < c->run_pool.size(); i++)
        if (c->run_pool[i].bytes >= bytes && (best < 0 || c->run_pool[i].bytes < c->run_pool[(size_t)best].bytes))
            best = (int)i;
    if (best >= 0) {
        DevBuf t = std::move(c->run_pool[(size_t)best]);
        c->run_pool.erase(c->run_pool.begin() + best);
        if (b.p) c->run_pool.push_back(std::move(b));
        b = std::move(t);
        return KC_OK;
    }
    return ensure(c, b, bytes);
}

// fin_packed's buffer leaves for a run (no copy); fin_packed gets a pooled
// buffer back if there is one (grown by the next finish if it is short)
DevBuf take_fin_packed(kc_ctx* c) {
    DevBuf run = std::move(c->fin_packed);
    if (!c->run_pool.empty()) {
        c->fin_packed = std::move(c->run_pool.back());
        c->run_pool.pop_back();
    }
    return run;
}

kc_status sync_stats(kc_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->stats_h, c->stats, ST_N * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

int32_t kc_abi_version(void) { return KC_ABI_VERSION; }

int32_t kc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* kc_strerror(kc_status s) {
    switch (s) {
    case KC_OK: return "ok";
    case KC_ERR_ARG: return "invalid argument";
    case KC_ERR_HIP: return "HIP runtime error";
    case KC_ERR_NOMEM: return "out of memory";
    case KC_ERR_FORMAT: return "malformed FASTQ block";
    case KC_ERR_IO: return "I/O error";
    case KC_ERR_STATE: return "invalid call for the context state";
    case KC_ERR_NODEVICE: return "no HIP device";
    case KC_ERR_INTERNAL: return "internal error";
    }
    return "unknown status";
}

const char* kc_last_error(const kc_ctx* c) { return c ? c->err.c_str() : ""; }

kc_status kc_create(kc_ctx** out, const kc_config* cfg) {
    if (!out || !cfg) return KC_ERR_ARG;
    *out = nullptr;
    if (cfg->kmer_length < 1 || cfg->kmer_length > KC_MAX_K) return KC_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return KC_ERR_NODEVICE;
    if (cfg->device < 0 || cfg->device >= ndev) return KC_ERR_NODEVICE;
    kc_ctx* c = new kc_ctx();
    c->cfg = *cfg;
    c->temp_dir = (cfg->temp_dir && cfg->temp_dir[0]) ? cfg->temp_dir : "";
    c->cfg.temp_dir = nullptr;
    c->k = cfg->kmer_length;
    c->W = (int)((c->k + 31) / 32);
    c->rs = 8 * c->W + 4;
    c->id = g_ctx_seq.fetch_add(1);
    memset(&c->st, 0, sizeof(c->st));
    kc_status s = KC_OK;
    auto bail = [&](kc_status e) {
        kc_destroy(c);
        return e;
    };
    if (hipSetDevice(cfg->device) != hipSuccess) return bail(KC_ERR_NODEVICE);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(KC_ERR_HIP);
    if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess || hipEventCreate(&c->evf[0]) != hipSuccess ||
        hipEventCreate(&c->evf[1]) != hipSuccess)
        return bail(KC_ERR_HIP);
    uint64_t M = cfg->gpu_memory_limit ? cfg->gpu_memory_limit : 100000000ull;
    if (M < (1u << 20)) M = 1u << 20;
    // (the table engine reads the text, not encoded reads)
    if ((cfg->flags & KC_FLAG_VARLEN) && (cfg->flags & KC_FLAG_ENGINE_TABLE)) return bail(KC_ERR_ARG);
    c->part = (cfg->flags & KC_FLAG_ENGINE_TABLE) == 0;
    c->skm = c->part && (cfg->flags & KC_FLAG_ENGINE_PREFIX) == 0;
    c->skm_force = (cfg->flags & KC_FLAG_ENGINE_SKM) != 0;
    size_t slot_bytes = 8 * (size_t)slot_words(c->W);
    size_t spill_bytes, tbytes;
    if (c->part) {
        // partition engine: two key buffers take the working set; the global
        // table and spill buffer only catch LDS-table overflow
        spill_bytes = M / 64;
        tbytes = cfg->table_bytes ? cfg->table_bytes : M / 16;
        uint64_t rest = M - M / 64 - M / 16;
        c->key_cap = rest / (16 * (uint64_t)c->W + 1);  // two key buffers + the P3 digit byte
        if (c->key_cap < 65536) c->key_cap = 65536;
    } else {
        spill_bytes = M / 16;
        tbytes = cfg->table_bytes ? cfg->table_bytes : (M - 4 * spill_bytes);
    }
    c->spill_cap = spill_bytes / (8 * c->W);
    if (c->spill_cap < 4096) c->spill_cap = 4096;
    c->cap = tbytes / slot_bytes;
    if (c->cap < 1024) c->cap = 1024;
    c->table_bytes = c->cap * slot_bytes;
    if (c->table.alloc(c->table_bytes) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->spill.alloc((size_t)c->spill_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->stats.alloc(ST_N * 8) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (hipHostMalloc((void**)&c->stats_h, ST_N * 8, 0) != hipSuccess) return bail(KC_ERR_NOMEM);
    if (c->part) {
        if (c->keys_a.alloc((size_t)c->key_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->keys_b.alloc((size_t)c->key_cap * 8 * c->W) != hipSuccess) return bail(KC_ERR_NOMEM);
        // key_cap digit bytes for the partition engine; the skm engine's two digit
        // arrays (2 x pool_cap, pool_cap = W key_cap / (W + 1)) with the second one
        // 16-byte aligned
        c->digs_bytes = c->key_cap;
        const uint64_t pool_max = (uint64_t)c->W * c->key_cap / (c->W + 1);
        if (((pool_max + 15) & ~15ull) + pool_max > c->digs_bytes) c->digs_bytes = ((pool_max + 15) & ~15ull) + pool_max;
        if (c->digs.alloc((size_t)c->digs_bytes + 16) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->rec_cursor.alloc(8) != hipSuccess) return bail(KC_ERR_NOMEM);
        if (c->pool_cursor.alloc(8) != hipSuccess) return bail(KC_ERR_NOMEM);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
            c->n_cu = prop.multiProcessorCount;
    }
    size_t mfree = 0, mtotal = 0;
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess) c->dev_total = mtotal;
    s = kc_reset(c);
    if (s) return bail(s);
    *out = c;
    return KC_OK;
}

// Ordered teardown of what is not a device buffer; the buffers go with the
// context object (every stream has been synchronised by then).
void kc_destroy(kc_ctx* c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    delete c->ring;  // waits for its DMAs
    delete c->pool;
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (char* b : c->file_bufs) (void)hipHostFree(b);
    for (char* b : c->acc_buf)
        if (b) (void)hipHostFree(b);
    if (c->stats_h) (void)hipHostFree(c->stats_h);
    for (auto* evs : {&c->acc_ev, &c->file_ev, &c->stage_free, &c->evf})
        for (hipEvent_t e : *evs)
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {c->ev0, c->ev1, c->ev2})
        if (e) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    for (auto& r : c->runs)
        if (!r.path.empty()) unlink(r.path.c_str());
    delete c;
}

kc_status kc_reset(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // the global table is cleared only when a slot was claimed since the last
    // clear (the partition engine's table is a rarely used fallback: clearing
    // 1/16 of gpuMemoryLimit per reset would cost milliseconds per count)
    kc_status s0 = sync_stats(c);
    if (s0) return s0;
    if (c->table_dirty || c->stats_h[ST_CLAIMED] > 0) {
        HIPCHK(c, hipMemsetAsync(c->table, 0, c->table_bytes, c->stream));
        c->table_dirty = false;
    }
    HIPCHK(c, hipMemsetAsync(c->stats, 0, ST_N * 8, c->stream));
    if (c->rec_cursor) HIPCHK(c, hipMemsetAsync(c->rec_cursor, 0, 8, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memset(c->stats_h, 0, ST_N * 8);
    // (acc_n: a DMA still reading an accumulation buffer is waited for before it is refilled)
    c->count = CountState();
    for (auto& r : c->runs)
        if (!r.path.empty()) unlink(r.path.c_str());
    c->runs.clear();
    release_dev_runs(c);
    memset(&c->st, 0, sizeof(c->st));
    c->st.table_capacity = c->cap;
    return KC_OK;
}

kc_status kc_copy_records(kc_ctx* c, void* dst, uint64_t dst_bytes) {
    if (!c || !dst) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: use kc_write_output");
    uint64_t bytes = c->count.n_records * c->rs;
    if (dst_bytes < bytes) return fail(c, KC_ERR_ARG, "destination holds %llu bytes, need %llu",
                                       (unsigned long long)dst_bytes, (unsigned long long)bytes);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (bytes) {
        HIPCHK(c, hipMemcpyAsync(dst, c->fin_packed.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return KC_OK;
}

kc_status kc_device_records(kc_ctx* c, const void** d_records, uint64_t* n_bytes) {
    if (!c || !d_records || !n_bytes) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    *d_records = c->fin_packed.p;
    *n_bytes = c->count.n_records * c->rs;
    return KC_OK;
}

// The finished table run (SortedKMerFile bytes) to host memory through the
// pinned ring, the pieces copied out by the pool while the next DMA runs.
static kc_status table_run_to_host(kc_ctx* c, std::vector<uint8_t>* mem) {
    const uint64_t bytes = c->count.n_records * c->rs;
    mem->resize(bytes);
    if (!bytes) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    kc_status s = stage_init(c);
    if (s) return s;
    uint8_t* dst = mem->data();
    HIPCHK(c, c->ring->download(c->fin_packed.p, bytes, c->stream, [&](const char* p, size_t n, size_t off) {
        kc::par_memcpy(c->pool, dst + off, p, n);
        return true;
    }));
    return KC_OK;
}

// The finished table run into a file at byte `at` (`whole`: the file is
// exactly the run, as after truncating it — the reference appends,
// KMerFileMerger.cpp:129): device -> pinned slot DMAs overlap the writes of
// the previous slot. An existing file is not truncated first but overwritten
// in place and cut to size at the end (truncating a cached file frees its
// pages, ~60 ms per GB, and the writes then allocate them again); the range
// is allocated up front (fallocate), the writes go out in 8 MiB pieces.
static kc_status table_run_to_file(kc_ctx* c, const char* path, uint64_t at = 0, bool whole = true) {
    const uint64_t bytes = c->count.n_records * c->rs;
    const double t0 = kc::trace_on() ? kc::now_s() : 0;
    int fd = open(path, O_CREAT | O_WRONLY, 0644);
    if (fd < 0) return fail(c, KC_ERR_IO, "cannot open output file %s: %s", path, strerror(errno));
    // the range is reserved up front: a full filesystem fails here, by name,
    // before any byte moves (filesystems without fallocate just write)
    if (bytes && fallocate(fd, 0, (off_t)at, (off_t)bytes) != 0 && errno != EOPNOTSUPP && errno != ENOSYS) {
        const int e = errno;
        close(fd);
        return fail(c, KC_ERR_IO, "cannot reserve %llu bytes at %llu in %s: %s", (unsigned long long)bytes,
                    (unsigned long long)at, path, strerror(e));
    }
    if (kc::trace_on()) kc::trace("output open + fallocate %.3f ms", (kc::now_s() - t0) * 1e3);
    kc_status s = KC_OK;
    if (bytes) {
        HIPCHK(c, hipSetDevice(c->cfg.device));
        if ((s = stage_init(c))) {
            close(fd);
            return s;
        }
        int werr = 0;
        uint64_t wat = 0;
        hipError_t e = c->ring->download(c->fin_packed.p, bytes, c->stream, [&](const char* p, size_t n, size_t off) {
            size_t done = 0;
            while (done < n) {
                const size_t piece = std::min((size_t)8 << 20, n - done);
                ssize_t w = pwrite(fd, p + done, piece, (off_t)(at + off + done));
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) {
                    werr = w < 0 ? errno : ENOSPC;  // a 0-byte write: no room
                    wat = at + off + done;
                    return false;
                }
                done += (size_t)w;
            }
            return true;
        });
        if (e == hipErrorUnknown)
            s = fail(c, KC_ERR_IO, "write to %s failed at byte %llu of %llu: %s", path, (unsigned long long)wat,
                     (unsigned long long)(at + bytes), strerror(werr));
        else if (e != hipSuccess) s = fail(c, KC_ERR_HIP, "output copy: %s", hipGetErrorString(e));
    }
    if (!s && whole && ftruncate(fd, (off_t)(at + bytes)) != 0)
        s = fail(c, KC_ERR_IO, "cannot size %s: %s", path, strerror(errno));
    if (close(fd) != 0 && !s) s = fail(c, KC_ERR_IO, "cannot close %s: %s", path, strerror(errno));
    if (kc::trace_on()) kc::trace("output %llu bytes in %.3f ms", (unsigned long long)bytes, (kc::now_s() - t0) * 1e3);
    return s;
}

kc_status kc_write_output(kc_ctx* c, const char* path, uint32_t fan_in, uint32_t threads) {
    if (!c || !path) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (c->runs.empty()) return table_run_to_file(c, path);
    std::vector<uint8_t> table_run;
    kc_status s = table_run_to_host(c, &table_run);
    if (s) return s;
    std::vector<RunSource> src;
    RunSource t;
    t.mem = table_run.data();
    t.bytes = table_run.size();
    src.push_back(t);
    for (auto& r : c->runs) {
        RunSource x;
        if (!r.path.empty())
            x.path = r.path;
        else {
            x.mem = r.mem.data();
            x.bytes = r.mem.size();
        }
        src.push_back(x);
    }
    std::string err;
    std::string tmp_prefix = std::string(path) + ".kctmp";
    if (!merge_tree(src, path, c->W, fan_in, threads, tmp_prefix, &err))
        return fail(c, KC_ERR_IO, "%s", err.c_str());
    return KC_OK;
}

kc_status kc_write_output_at(kc_ctx* c, const char* path, uint64_t offset) {
    if (!c || !path) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: use kc_write_output");
    return table_run_to_file(c, path, offset, false);
}

kc_status kc_write_runs(kc_ctx* c, const char* prefix, uint32_t* n_runs) {
    if (!c || !prefix) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    std::vector<uint8_t> table_run;
    kc_status s = table_run_to_host(c, &table_run);
    if (s) return s;
    uint32_t count = 0;
    auto write_one = [&](const uint8_t* p, size_t bytes, const std::string& from) -> kc_status {
        std::string name = std::string(prefix) + "." + std::to_string(count);
        if (!from.empty()) {
            // copy the temp file
            FILE* in = fopen(from.c_str(), "rb");
            FILE* out = fopen(name.c_str(), "wb");
            if (!in || !out) {
                if (in) fclose(in);
                if (out) fclose(out);
                return fail(c, KC_ERR_IO, "cannot copy run %s to %s: %s", from.c_str(), name.c_str(), strerror(errno));
            }
            std::vector<char> buf(1 << 20);
            size_t got;
            while ((got = fread(buf.data(), 1, buf.size(), in)) > 0) fwrite(buf.data(), 1, got, out);
            fclose(in);
            fclose(out);
        } else {
            FILE* out = fopen(name.c_str(), "wb");
            if (!out) return fail(c, KC_ERR_IO, "cannot write run %s: %s", name.c_str(), strerror(errno));
            size_t w = bytes ? fwrite(p, 1, bytes, out) : 0;
            const int we = errno;
            const int ce = fclose(out) != 0 ? errno : 0;
            if (w != bytes || ce) return fail(c, KC_ERR_IO, "short write %s: %s", name.c_str(), strerror(w != bytes ? we : ce));
        }
        count++;
        return KC_OK;
    };
    if ((s = write_one(table_run.data(), table_run.size(), ""))) return s;
    for (auto& r : c->runs)
        if ((s = write_one(r.mem.data(), r.mem.size(), r.path))) return s;
    if (n_runs) *n_runs = count;
    return KC_OK;
}

kc_status kc_get_stats(const kc_ctx* c, kc_stats* out) {
    if (!c || !out) return KC_ERR_ARG;
    *out = c->st;
    out->insert_launches = c->count.insert_launches;
    out->insert_ms = c->count.insert_ms;
    for (int i = 0; i < 5; i++) out->part_ms[i] = c->count.part_ms[i];
    out->presplit_ms = c->count.presplit_ms;
    out->presplit_batches = c->count.presplit_batches;
    out->sorted_run_batches = c->count.sorted_run_batches;
    out->key_passes = c->count.key_passes;
    out->batches = c->count.batches_cut + c->count.batches;
    out->keys = c->count.part_keys;
    out->p5_launches = c->count.p5_launches;
    out->table_capacity = c->cap;
    out->valid_kmers = c->stats_h[ST_VALID];
    out->spill_runs = c->count.runs_cut + c->runs.size();
    out->engines_used = c->count.engines_used;
    out->dedup_ms = c->count.dedup_ms;
    out->dedup_records = c->stats_h[ST_DEDUP];
    out->finish_group_ms = c->count.finish_group_ms;
    return KC_OK;
}

kc_status kc_merge_files(const char* const* inputs, uint32_t n_inputs, const char* output, int64_t kmer_length,
                         uint32_t fan_in, uint32_t threads) {
    if (!output || kmer_length < 1 || kmer_length > KC_MAX_K || (n_inputs && !inputs)) return KC_ERR_ARG;
    int W = (int)((kmer_length + 31) / 32);
    std::vector<RunSource> src;
    for (uint32_t i = 0; i < n_inputs; i++) {
        RunSource r;
        r.path = inputs[i];
        src.push_back(r);
    }
    std::string err;
    if (!merge_tree(src, output, W, fan_in, threads, std::string(output) + ".kctmp", &err)) return KC_ERR_IO;
    return KC_OK;
}

struct kc_merge_part {
    kc::MergedPart part;
};

kc_status kc_merge_part_create(const char* const* inputs, uint32_t n_inputs, int64_t kmer_length, uint32_t part,
                               uint32_t parts, uint32_t threads, kc_merge_part** out, uint64_t* n_bytes) {
    if (!out || kmer_length < 1 || kmer_length > KC_MAX_K || (n_inputs && !inputs) || parts < 1 || part >= parts)
        return KC_ERR_ARG;
    *out = nullptr;
    const int W = (int)((kmer_length + 31) / 32);
    std::vector<RunSource> src;
    for (uint32_t i = 0; i < n_inputs; i++) {
        if (!inputs[i]) return KC_ERR_ARG;
        RunSource r;
        r.path = inputs[i];
        src.push_back(r);
    }
    std::unique_ptr<kc_merge_part> p(new (std::nothrow) kc_merge_part());
    if (!p) return KC_ERR_NOMEM;
    int e = 0;
    try {
        if (!kc::merge_runs_part(src, W, part, parts, threads ? threads : 1, &p->part, &e)) return KC_ERR_IO;
    } catch (const std::bad_alloc&) {
        return KC_ERR_NOMEM;
    }
    if (n_bytes) *n_bytes = p->part.bytes;
    *out = p.release();
    return KC_OK;
}

kc_status kc_merge_part_write(kc_merge_part* p, const char* output, uint64_t offset, uint64_t file_bytes) {
    if (!p || !output) return KC_ERR_ARG;
    if (file_bytes && offset + p->part.bytes > file_bytes) return KC_ERR_ARG;
    return kc::write_part_at(p->part, output, offset, file_bytes) ? KC_OK : KC_ERR_IO;
}

void kc_merge_part_destroy(kc_merge_part* p) { delete p; }

uint64_t kc_synth_fastq_bytes(const kc_synth_spec* sp) {
    if (!sp) return 0;
    return synth_bytes(sp->first_read, sp->n_reads, sp->read_length, (int)sp->layout);
}

static SynthArgs synth_args(const kc_synth_spec* sp) {
    SynthArgs a;
    a.first = sp->first_read;
    a.n = sp->n_reads;
    a.seed = sp->seed;
    a.genome = sp->genome_length;
    a.L = sp->read_length;
    a.Lmin = sp->min_read_length;
    a.layout = (int)sp->layout;
    double thr = sp->n_rate * 9007199254740992.0;
    a.n_threshold = sp->n_rate <= 0 ? 0 : (thr >= 9007199254740992.0 ? (1ull << 53) : (uint64_t)thr);
    return a;
}

static bool synth_ok(const kc_synth_spec* sp) {
    return sp && sp->read_length > 0 && (sp->genome_length == 0 || sp->genome_length >= (uint64_t)sp->read_length) &&
           sp->min_read_length >= 0 && sp->min_read_length <= sp->read_length && sp->layout <= 1 &&
           (sp->layout == 0 || sp->min_read_length == 0 || sp->min_read_length == sp->read_length);
}

kc_status kc_synth_fastq_host(const kc_synth_spec* sp, char* dst, uint64_t dst_bytes) {
    if (!synth_ok(sp) || !dst) return KC_ERR_ARG;
    if (dst_bytes < kc_synth_fastq_bytes(sp)) return KC_ERR_ARG;
    synth_host(synth_args(sp), dst);
    return KC_OK;
}

kc_status kc_synth_fastq_device(kc_ctx* c, const kc_synth_spec* sp, void** d_out, uint64_t* n_bytes) {
    if (!c || !synth_ok(sp) || !d_out) return KC_ERR_ARG;
    uint64_t bytes = kc_synth_fastq_bytes(sp);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, bytes + 64));
    HIPCHK(c, launch_synth(synth_args(sp), (char*)p, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d_out = p;
    if (n_bytes) *n_bytes = bytes;
    return KC_OK;
}

kc_status kc_synth_free(kc_ctx* c, void* d_buf) {
    if (!c) return KC_ERR_ARG;
    if (d_buf) HIPCHK(c, hipFree(d_buf));
    return KC_OK;
}

kc_status kc_owner_counts(kc_ctx* c, uint32_t world, uint64_t* counts) {
    if (!c || world == 0 || !counts) return KC_ERR_ARG;
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: the key-space exchange needs one run");
    kc_status s;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->part_starts, ((size_t)world + 1) * 8))) return s;
    HIPCHK(c, launch_owner_bounds(c->fin_packed.p, c->rs, c->count.n_records, world, c->part_starts.as<uint64_t>(), c->stream));
    std::vector<uint64_t> b(world + 1);
    HIPCHK(c, hipMemcpyAsync(b.data(), c->part_starts.p, (world + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t o = 0; o < world; o++) counts[o] = b[o + 1] - b[o];
    return KC_OK;
}


// ---- queries on the finished run ------------------------------------------

// The state rules the queries share with kc_copy_records.
static kc_status query_state(kc_ctx* c) {
    if (!c->count.finished) return fail(c, KC_ERR_STATE, "call kc_finish first");
    if (!c->runs.empty()) return fail(c, KC_ERR_STATE, "spill runs exist: write the output and use the file form");
    return KC_OK;
}

kc_status kc_count_histogram(kc_ctx* c, uint64_t* bins, uint32_t n_bins) {
    if (!c || !bins) return KC_ERR_ARG;
    if (n_bins < 2 || n_bins > 65536) return fail(c, KC_ERR_ARG, "n_bins %u outside [2, 65536]", n_bins);
    kc_status s;
    if ((s = query_state(c))) return s;
    memset(bins, 0, (size_t)n_bins * 8);
    if (c->count.n_records == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->q_bins, (size_t)n_bins * 8 + 8))) return s;
    HIPCHK(c, hipMemsetAsync(c->q_bins.p, 0, (size_t)n_bins * 8, c->stream));
    HIPCHK(c, launch_count_histo(c->fin_packed.p, c->W, c->count.n_records, n_bins, c->q_bins.as<uint64_t>(), c->stream));
    HIPCHK(c, hipMemcpyAsync(bins, c->q_bins.p, (size_t)n_bins * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_filter_records(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t* n_kept) {
    if (!c) return KC_ERR_ARG;
    if (min_count > max_count) return fail(c, KC_ERR_ARG, "min_count %u > max_count %u", min_count, max_count);
    kc_status s;
    if ((s = query_state(c))) return s;
    const uint64_t n = c->count.n_records;
    if (n_kept) *n_kept = n;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    // tile counts, their exclusive scan, the scan's scratch, the total
    const uint64_t ntiles = (n + filter_tile() - 1) / filter_tile();
    if ((s = ensure(c, c->q_tiles, (2 * ntiles + scan_tmp_elems(ntiles) + 1) * 8))) return s;
    uint64_t* cnt = c->q_tiles.as<uint64_t>();
    uint64_t* base = cnt + ntiles;
    uint64_t* total = base + ntiles;
    uint64_t* tmp = total + 1;
    HIPCHK(c, launch_filter_count(c->fin_packed.p, c->W, n, min_count, max_count, cnt, c->stream));
    HIPCHK(c, launch_scan_u64(cnt, base, ntiles, tmp, c->stream));
    HIPCHK(c, launch_sum_last(base, cnt, ntiles, total, c->stream));
    uint64_t kept = 0;
    HIPCHK(c, hipMemcpyAsync(&kept, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (kept > n) return fail(c, KC_ERR_INTERNAL, "filter kept %llu of %llu records", (unsigned long long)kept,
                              (unsigned long long)n);
    if (kept != 0 && kept != n) {
        // out of place: the kept records into a pooled buffer that becomes the
        // run; the old buffer joins the pool, as kc_finish and the merges do
        DevBuf dst;
        if ((s = ensure_pooled(c, dst, (size_t)kept * c->rs + 16))) return s;
        hipError_t e = launch_filter_scatter(c->fin_packed.p, c->W, n, min_count, max_count, base, dst.p, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            c->run_pool.push_back(std::move(dst));
            return fail(c, KC_ERR_HIP, "filter scatter: %s", hipGetErrorString(e));
        }
        c->run_pool.push_back(std::move(c->fin_packed));
        c->fin_packed = std::move(dst);
    }
    c->count.n_records = kept;
    c->st.output_records = kept;
    if (n_kept) *n_kept = kept;
    return KC_OK;
}

kc_status kc_lookup_device(kc_ctx* c, const void* d_keys, uint64_t n_keys, void* d_counts, void* d_found,
                           uint64_t* n_found) {
    if (!c || (n_keys && (!d_keys || !d_counts))) return KC_ERR_ARG;
    kc_status s;
    if ((s = query_state(c))) return s;
    if (n_found) *n_found = 0;
    if (n_keys == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if ((s = ensure(c, c->q_bins, 8))) return s;
    HIPCHK(c, hipMemsetAsync(c->q_bins.p, 0, 8, c->stream));
    HIPCHK(c, launch_lookup(c->fin_packed.p, c->W, c->count.n_records, (const uint64_t*)d_keys, n_keys, (uint32_t*)d_counts,
                            (uint8_t*)d_found, c->q_bins.as<uint64_t>(), c->stream));
    uint64_t nf = 0;
    HIPCHK(c, hipMemcpyAsync(&nf, c->q_bins.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_found) *n_found = nf;
    return KC_OK;
}

kc_status kc_lookup(kc_ctx* c, const uint64_t* keys, uint64_t n_keys, uint32_t* counts, uint8_t* found,
                    uint64_t* n_found) {
    if (!c || (n_keys && (!keys || !counts))) return KC_ERR_ARG;
    kc_status s;
    if ((s = query_state(c))) return s;
    if (n_found) *n_found = 0;
    if (n_keys == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t kb = (size_t)n_keys * c->W * 8;
    if ((s = ensure(c, c->q_keys, kb)) || (s = ensure(c, c->q_counts, (size_t)n_keys * 4)) ||
        (s = ensure(c, c->q_found, (size_t)n_keys)))
        return s;
    HIPCHK(c, hipMemcpyAsync(c->q_keys.p, keys, kb, hipMemcpyHostToDevice, c->stream));
    if ((s = kc_lookup_device(c, c->q_keys.p, n_keys, c->q_counts.p, c->q_found.p, n_found))) return s;
    HIPCHK(c, hipMemcpyAsync(counts, c->q_counts.p, (size_t)n_keys * 4, hipMemcpyDeviceToHost, c->stream));
    if (found) HIPCHK(c, hipMemcpyAsync(found, c->q_found.p, (size_t)n_keys, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_histogram_file(const char* path, int64_t kmer_length, uint64_t* bins, uint32_t n_bins) {
    if (!path || !bins || kmer_length < 1 || kmer_length > KC_MAX_K || n_bins < 2 || n_bins > 65536)
        return KC_ERR_ARG;
    return kc::histogram_file(path, (int)((kmer_length + 31) / 32), bins, n_bins) ? KC_OK : KC_ERR_IO;
}

kc_status kc_filter_file(const char* input, const char* output, int64_t kmer_length, uint32_t min_count,
                         uint32_t max_count, uint64_t* n_kept) {
    if (!input || !output || kmer_length < 1 || kmer_length > KC_MAX_K || min_count > max_count) return KC_ERR_ARG;
    return kc::filter_file(input, output, (int)((kmer_length + 31) / 32), min_count, max_count, n_kept) ? KC_OK
                                                                                                         : KC_ERR_IO;
}

kc_status kc_canonicalize_file(const char* input, const char* output, int64_t kmer_length, uint64_t* n_records) {
    if (!input || !output || kmer_length < 1 || kmer_length > KC_MAX_K) return KC_ERR_ARG;
    return kc::canonicalize_file(input, output, (int)kmer_length, n_records) ? KC_OK : KC_ERR_IO;
}

// ---- set operations between two finished runs ------------------------------

static bool setop_ok(uint32_t op, uint32_t mode) {
    if (op > KC_SET_COUNT_SUBTRACT || mode > KC_SETC_RIGHT) return false;
    return op <= KC_SET_INTERSECT || mode == KC_SETC_SUM;
}

// `dst` (a pooled buffer that holds the result) becomes the finished run of
// n records; the old run joins the pool, as after kc_filter_records.
static void install_run(kc_ctx* c, DevBuf& dst, uint64_t n) {
    if (dst.p) {
        if (c->fin_packed.p) c->run_pool.push_back(std::move(c->fin_packed));
        c->fin_packed = std::move(dst);
    }
    c->count.n_records = n;
    c->st.output_records = n;
}

kc_status kc_combine_records_device(kc_ctx* c, const void* d_packed, uint64_t n_records, uint32_t op,
                                    uint32_t count_mode, uint64_t* n_out) {
    if (!c || (n_records && !d_packed)) return KC_ERR_ARG;
    if (!setop_ok(op, count_mode)) return fail(c, KC_ERR_ARG, "set operation %u with count mode %u", op, count_mode);
    kc_status s;
    if ((s = query_state(c))) return s;
    const uint64_t na = c->count.n_records, nb = n_records;
    const size_t rs = (size_t)c->rs;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    DevBuf dst;
    uint64_t nout = 0;
    if (na == 0 || nb == 0) {
        // an empty operand: nothing to merge. The result is A, B or empty.
        if (nb == 0 && op != KC_SET_INTERSECT) {
            nout = na;
        } else if (na == 0 && op == KC_SET_UNION) {
            if ((s = ensure_pooled(c, dst, (size_t)nb * rs + 16))) return s;
            hipError_t e = hipMemcpyAsync(dst.p, d_packed, (size_t)nb * rs, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) {
                c->run_pool.push_back(std::move(dst));
                return fail(c, KC_ERR_HIP, "combine copy: %s", hipGetErrorString(e));
            }
            nout = nb;
        }
        install_run(c, dst, nout);
        if (n_out) *n_out = nout;
        return KC_OK;
    }
    const uint64_t n = na + nb;
    const uint64_t ntiles = (n + (uint64_t)setop_tile(c->W) - 1) / (uint64_t)setop_tile(c->W);
    // the tile splits; tile counts, their exclusive scan, the total, the scan's scratch
    if ((s = ensure(c, c->fin_misc, merge_packed_split_elems(c->W, n) * 8)) ||
        (s = ensure(c, c->q_tiles, (2 * ntiles + scan_tmp_elems(ntiles) + 1) * 8)))
        return s;
    uint64_t* split = c->fin_misc.as<uint64_t>();
    uint64_t* cnt = c->q_tiles.as<uint64_t>();
    uint64_t* base = cnt + ntiles;
    uint64_t* total = base + ntiles;
    uint64_t* tmp = total + 1;
    HIPCHK(c, launch_setop_count(c->W, c->fin_packed.p, na, d_packed, nb, op, count_mode, split, cnt, c->stream));
    HIPCHK(c, launch_scan_u64(cnt, base, ntiles, tmp, c->stream));
    HIPCHK(c, launch_sum_last(base, cnt, ntiles, total, c->stream));
    HIPCHK(c, hipMemcpyAsync(&nout, total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nout > n) return fail(c, KC_ERR_INTERNAL, "combine kept %llu of %llu records", (unsigned long long)nout,
                              (unsigned long long)n);
    if (nout) {
        if ((s = ensure_pooled(c, dst, (size_t)nout * rs + 16))) return s;
        hipError_t e = launch_setop_emit(c->W, c->fin_packed.p, na, d_packed, nb, op, count_mode, split, base, dst.p,
                                         c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            c->run_pool.push_back(std::move(dst));
            return fail(c, KC_ERR_HIP, "combine emit: %s", hipGetErrorString(e));
        }
    }
    install_run(c, dst, nout);
    if (n_out) *n_out = nout;
    return KC_OK;
}

kc_status kc_combine_contexts(kc_ctx* a, kc_ctx* b, uint32_t op, uint32_t count_mode, uint64_t* n_out) {
    if (!a || !b) return KC_ERR_ARG;
    if (a == b) return fail(a, KC_ERR_ARG, "combine: both operands are the same context");
    if (a->k != b->k) return fail(a, KC_ERR_ARG, "combine: kmer_length %lld and %lld", (long long)a->k, (long long)b->k);
    if (!setop_ok(op, count_mode)) return fail(a, KC_ERR_ARG, "set operation %u with count mode %u", op, count_mode);
    kc_status s;
    if ((s = query_state(a))) return s;
    if (query_state(b)) return fail(a, KC_ERR_STATE, "combine: the second context: %s", b->err.c_str());
    const uint64_t nb = b->count.n_records;
    if (a->cfg.device == b->cfg.device || nb == 0)
        return kc_combine_records_device(a, nb ? b->fin_packed.p : nullptr, nb, op, count_mode, n_out);
    // b's run comes over to a's device, as kc_gather_contexts copies runs
    HIPCHK(a, hipSetDevice(a->cfg.device));
    DevBuf recv;
    HIPCHK(a, recv.alloc((size_t)nb * a->rs + 16));
    HIPCHK(a, hipMemcpyPeerAsync(recv.p, a->cfg.device, b->fin_packed.p, b->cfg.device, (size_t)nb * a->rs, a->stream));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    return kc_combine_records_device(a, recv.p, nb, op, count_mode, n_out);
}

kc_status kc_combine_files(const char* a, const char* b, const char* output, int64_t kmer_length, uint32_t op,
                           uint32_t count_mode, uint64_t* n_out) {
    if (!a || !b || !output || kmer_length < 1 || kmer_length > KC_MAX_K || !setop_ok(op, count_mode))
        return KC_ERR_ARG;
    return kc::combine_files(a, b, output, (int)((kmer_length + 31) / 32), op, count_mode, n_out) ? KC_OK : KC_ERR_IO;
}

kc_status kc_copy_device(kc_ctx* c, void* d_dst, const void* d_src, uint64_t n) {
    if (!c || (n && (!d_dst || !d_src))) return KC_ERR_ARG;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(d_dst, d_src, n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

kc_status kc_copy_to_host(kc_ctx* c, void* dst, const void* d_src, uint64_t n) {
    if (!c || (n && (!dst || !d_src))) return KC_ERR_ARG;
    if (n == 0) return KC_OK;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}
