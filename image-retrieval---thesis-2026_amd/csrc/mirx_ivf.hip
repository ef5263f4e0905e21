// mirx_ivf.hip -- the IVF indexes of the C ABI (include/mirx.h, mirx_ivf_*): k-means lists over a flat index of the centroids,
// the list-major master (fp32 rows for IVF_FLAT, 8-bit codes for IVF_SQ8, m codeword numbers for IVF_PQ), and the search of the
// probed lists (kernels: k_ivf.hip, k_ivf_pq.hip).
//
// "Nearest centroid" is never restated here: assignments and probes are mirx_index_search / mirx_index_rank_top over `cent`, a
// mirx_index that holds the centroids with ids 0 .. nlist-1, so the rule (fp64 lane-tree score, ties to the lowest list) is the
// one oracle/search_ref.c pins.  The layout is planned on the host -- list numbers and ids travel there (8 bytes per row), a
// counting sort gives every row its destination, the device moves the rows -- which keeps add / remove / re-assign free of
// order-dependent atomics at a cost that is stated in the header.
#include <algorithm>
#include <new>
#include <numeric>
#include <unordered_set>
#include <vector>

#include "mirx_kernels.h"

using namespace mirx;

struct mirx_ivf {
    int dim = 0, dimp = 0, metric = 0, device = 0, nlist = 0, kind = MIRX_IVF_FLAT;
    mirx_index *cent = nullptr;           // flat index over the centroids; null until they are fixed
    DevBuf centroids;                     // [nlist, dim] fp32
    int64_t size = 0;
    DevBuf rows, ids, offsets;            // [size, dimp] list-major (fp32, or uint8 codes for SQ8), [size], [nlist + 1] int64
    std::vector<int64_t> off_h, ids_h, seq_h;   // host mirrors of offsets / ids, and each row's insertion number (list-major)
    int64_t next_seq = 0, next_auto = 0;
    int64_t score_bytes = 0;              // MIRX_IVF_OPT_SCORE_BYTES; 0 = SCORE_WS_BYTES
    unsigned long long *stats_dev = nullptr;   // [3] rows scored, pairs, work items
    int64_t last_nq = 0, last_batches = 0;
    // scratch of every kind: train / add / remove, then the search loop's common workspace
    DevBuf stage, lists, fval, a_order, a_loff, upd, pos, newids, pids, probes, qoff, cntcur, itemoff, scores;
    // scratch of the row scan (FLAT, SQ8): a PQ handle never touches these
    DevBuf q32p, pairoff, pair_q, pair_off;

    // ---- SQ8 only ----
    DevBuf range;                         // vmin [dimp] then scale [dimp] fp32, zero in the padding
    bool range_fixed = false;

    // ---- PQ only: a FLAT or SQ8 handle never touches anything below ----
    int pq_m = 0;                         // sub-quantisers; a code row is pq_m bytes
    DevBuf codebooks;                     // [pq_m][256][dim / pq_m] fp32
    bool cb_fixed = false;
    bool pq_res = false;                  // residual coding (mirx_ivf_create_pq_ex): codes of row - centroid of its list
    DevBuf norms;                         // residual PQ under L2: N2 [size] fp64, list-major beside ids
    // PQ's scratch: the search's tables, bases and |q|^2; the encoder's sub-vectors, found codewords and residual chunk; add's
    // new codes, lists and norms
    DevBuf tables, pq_base, pq_qq, pq_sub, pq_found, pq_resid, pq_codes, pq_lists, pq_n2;

    bool sq8() const { return kind == MIRX_IVF_SQ8; }
    bool pq() const { return kind == MIRX_IVF_PQ; }
    bool res_l2() const { return pq() && pq_res && metric != MIRX_METRIC_IP; }     // the handles that keep N2
    int code_ld() const { return pq() ? pq_m : dimp; }                             // bytes of a code row (SQ8, PQ)
    size_t row_bytes() const { return pq() ? (size_t)pq_m : (size_t)dimp * (sq8() ? 1 : sizeof(float)); }
    const float *vmin() const { return range.as<float>(); }
    const float *scale() const { return range.as<float>() + dimp; }
};

namespace {

constexpr size_t SCORE_WS_BYTES = (size_t)1 << 30;
constexpr int64_t MAX_BATCH_PAIRS = (int64_t)1 << 26;   // (query, probe) pairs of one internal batch

#define MIRX_IVF_ENTER(ivf, who)                                                        \
    MIRX_CHECK(ivf, std::string(who) + ": null ivf");                                   \
    DeviceGuard dg((ivf)->device);                                                      \
    if (!dg.ok) return fail(MIRX_EHIP, std::string(who) + ": cannot select the ivf's device")

#define MIRX_IVF_SQ8_ONLY(ivf, who) MIRX_CHECK((ivf)->sq8(), std::string(who) + ": the ivf is not MIRX_IVF_SQ8")
#define MIRX_IVF_PQ_ONLY(ivf, who) MIRX_CHECK((ivf)->pq(), std::string(who) + ": the ivf is not MIRX_IVF_PQ")
#define MIRX_IVF_CODED_ONLY(ivf, who) MIRX_CHECK((ivf)->sq8() || (ivf)->pq(), std::string(who) + ": the ivf is not MIRX_IVF_SQ8 or MIRX_IVF_PQ")

// the trained parts a call needs fixed (trained_parts_fixed): the centroids of every kind, SQ8's range, PQ's codebooks
enum : unsigned { CENTROIDS = 1, RANGE = 2, CODEBOOKS = 4, ALL_PARTS = CENTROIDS | RANGE | CODEBOOKS };

// MIRX_ESTATE naming the first of `need` that this handle's kind has and that is not fixed yet
int trained_parts_fixed(const mirx_ivf *ivf, const char *who, unsigned need) {
    if ((need & CENTROIDS) && !ivf->cent)
        return fail(MIRX_ESTATE, std::string(who) + ": the centroids are not fixed yet (mirx_ivf_train / _set_centroids)");
    if ((need & RANGE) && ivf->sq8() && !ivf->range_fixed)
        return fail(MIRX_ESTATE, std::string(who) + ": the range is not fixed yet (mirx_ivf_sq8_train / _sq8_set_range)");
    if ((need & CODEBOOKS) && ivf->pq() && !ivf->cb_fixed)
        return fail(MIRX_ESTATE, std::string(who) + ": the codebooks are not fixed yet (mirx_ivf_pq_train / _pq_set_codebooks)");
    return MIRX_OK;
}

// SQ8 and PQ keep no originals: what would re-assign or re-encode the resident rows is refused
int coded_rows_keep_trained_parts(const mirx_ivf *ivf, const char *who) {
    if (ivf->sq8() && ivf->size > 0)
        return fail(MIRX_ESTATE, std::string(who) + ": an IVF_SQ8 index that holds rows keeps its centroids and range (the original rows are gone)");
    if (ivf->pq() && ivf->size > 0)
        return fail(MIRX_ESTATE, std::string(who) + ": an IVF_PQ index that holds rows keeps its centroids and codebooks (the original rows are gone)");
    return MIRX_OK;
}

// rows as a device pointer: the caller's, or a copy in `buf`
int device_rows(mirx_ivf *ivf, const float *rows, int64_t n, DevBuf &buf, const float **out) {
    *out = rows;
    if (is_device_pointer(rows)) return MIRX_OK;
    const size_t bytes = (size_t)n * ivf->dim * sizeof(float);
    if (buf.ensure(bytes) != hipSuccess) return fail(MIRX_ENOMEM, "ivf: no memory to stage the rows");
    MIRX_HIP(hipMemcpy(buf.p, rows, bytes, hipMemcpyHostToDevice));
    *out = buf.as<float>();
    return MIRX_OK;
}

// the flat index over the current centroids (ids = list numbers)
int rebuild_centroid_index(mirx_ivf *ivf) {
    if (ivf->cent) mirx_index_destroy(ivf->cent);
    ivf->cent = nullptr;
    if (int rc = mirx_index_create(ivf->dim, ivf->metric, ivf->device, &ivf->cent)) return rc;
    return mirx_index_add(ivf->cent, ivf->centroids.as<float>(), ivf->nlist, nullptr);
}

// out_lists[i] (device) = the list of rows[i] (device, [n, dim]); the work is enqueued on st, mirx_index_search waits as it does
int assign_rows(mirx_ivf *ivf, const float *rows, int64_t n, int64_t *out_lists, hipStream_t st) {
    if (n == 0) return MIRX_OK;
    MIRX_HIP(ivf->fval.ensure((size_t)n * sizeof(float)));
    return mirx_index_search(ivf->cent, rows, n, 1, nullptr, ivf->fval.as<float>(), out_lists, st);
}

// to the host: for every row the nearest of `ix`'s nlist rows (ids 0 .. nlist-1), by ix's own search
int nearest_to_host(mirx_ivf *ivf, mirx_index *ix, int nlist, const float *rows, int64_t n, std::vector<int64_t> &out,
                    hipStream_t st) {
    out.resize((size_t)n);
    if (n == 0) return MIRX_OK;
    MIRX_HIP(ivf->lists.ensure((size_t)n * sizeof(int64_t)));
    MIRX_HIP(ivf->fval.ensure((size_t)n * sizeof(float)));
    if (int rc = mirx_index_search(ix, rows, n, 1, nullptr, ivf->fval.as<float>(), ivf->lists.as<int64_t>(), st)) return rc;
    MIRX_HIP(hipMemcpyAsync(out.data(), ivf->lists.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    MIRX_HIP(hipStreamSynchronize(st));
    for (int64_t v : out)
        if (v < 0 || v >= nlist) return fail(MIRX_EHIP, "ivf: the centroid search returned no list for a row");
    return MIRX_OK;
}

// the list of every row, to the host
int assign_to_host(mirx_ivf *ivf, const float *rows, int64_t n, std::vector<int64_t> &out, hipStream_t st) {
    return nearest_to_host(ivf, ivf->cent, ivf->nlist, rows, n, out, st);
}

// a flat index over rows [n, dim] (device) with ids 0 .. n-1
int flat_over(int dim, int metric, int device, const float *rows, int n, mirx_index **out) {
    *out = nullptr;
    if (int rc = mirx_index_create(dim, metric, device, out)) return rc;
    if (int rc = mirx_index_add(*out, rows, n, nullptr)) {
        mirx_index_destroy(*out);
        *out = nullptr;
        return rc;
    }
    return MIRX_OK;
}

// Lloyd's loop of mirx_ivf_train over rows [n, dim] (device): cent [nlist, dim] (device) starts at rows[start[.]], then at most
// `iters` updates, stopping when an assignment pass changes no row's list.  "Nearest" is a flat index over the current centroids.
int lloyd(mirx_ivf *ivf, const float *drows, int64_t n, int dim, int metric, int nlist, const std::vector<int64_t> &start,
          int iters, float *cent, hipStream_t st) {
    MIRX_HIP(ivf->pos.ensure((size_t)nlist * sizeof(int64_t)));
    MIRX_HIP(ivf->upd.ensure((size_t)nlist * dim * sizeof(float)));
    MIRX_HIP(ivf->a_order.ensure((size_t)n * sizeof(int32_t)));
    MIRX_HIP(ivf->a_loff.ensure((size_t)(nlist + 1) * sizeof(int64_t)));
    MIRX_HIP(hipMemcpyAsync(ivf->pos.p, start.data(), (size_t)nlist * sizeof(int64_t), hipMemcpyHostToDevice, st));
    MIRX_HIP(launch_ivf_place(drows, nlist, dim, dim, ivf->pos.as<int64_t>(), nullptr, cent, dim, st));
    MIRX_HIP(hipStreamSynchronize(st));
    std::vector<int64_t> cur, prev, loff((size_t)nlist + 1);
    std::vector<int32_t> order((size_t)n);
    for (int it = 0; it < iters; ++it) {
        mirx_index *ix = nullptr;
        if (int rc = flat_over(dim, metric, ivf->device, cent, nlist, &ix)) return rc;
        const int rc = nearest_to_host(ivf, ix, nlist, drows, n, cur, st);
        mirx_index_destroy(ix);
        if (rc) return rc;
        if (it > 0 && cur == prev) break;
        std::fill(loff.begin(), loff.end(), 0);
        for (int64_t v : cur) ++loff[(size_t)v + 1];
        for (int l = 0; l < nlist; ++l) loff[(size_t)l + 1] += loff[(size_t)l];
        std::vector<int64_t> at(loff.begin(), loff.end() - 1);
        for (int64_t r = 0; r < n; ++r) order[(size_t)at[(size_t)cur[(size_t)r]]++] = (int32_t)r;
        MIRX_HIP(hipMemcpyAsync(ivf->a_order.p, order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
        MIRX_HIP(hipMemcpyAsync(ivf->a_loff.p, loff.data(), (size_t)(nlist + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        MIRX_HIP(launch_ivf_update(drows, dim, ivf->a_order.as<int32_t>(), ivf->a_loff.as<int64_t>(), nlist, cent,
                                   ivf->upd.as<float>(), metric == MIRX_METRIC_IP, st));
        MIRX_HIP(hipStreamSynchronize(st));
        prev.swap(cur);
    }
    return MIRX_OK;
}

// ---- IVF_PQ's quantiser: "nearest codeword" is mirx_index_search(k = 1) over a sub-space's 256 codewords, never restated --------
bool pq_shape_ok(int dim, int m) {
    return m >= 4 && m <= PQ_MAX_M && m % 4 == 0 && dim >= 1 && dim <= MIRX_IVF_MAX_DIM && dim % (4 * m) == 0;
}

void free_codeword_indexes(std::vector<mirx_index *> &v) {
    for (mirx_index *ix : v)
        if (ix) mirx_index_destroy(ix);
    v.clear();
}

// per sub-space a flat L2 index over its codewords; cb = device [m][256][dim / m]
int build_codeword_indexes(int dim, int m, int device, const float *cb, std::vector<mirx_index *> &out) {
    free_codeword_indexes(out);
    const int dsub = dim / m;
    for (int j = 0; j < m; ++j) {
        mirx_index *ix = nullptr;
        if (int rc = flat_over(dsub, MIRX_METRIC_NEG_L2, device, cb + (size_t)j * 256 * dsub, 256, &ix)) {
            free_codeword_indexes(out);
            return rc;
        }
        out.push_back(ix);
    }
    return MIRX_OK;
}

constexpr int64_t PQ_ENCODE_CHUNK = (int64_t)1 << 16;   // rows per pass of the encoder: bounds its scratch and the m indexes' workspaces

// residual coding for the encoder: row i is coded as rows[i] - cent[lists[i]] (lists: device, [n]); buf holds one chunk of residuals
struct PqResidual {
    const int64_t *lists;
    const float *cent;
    int nlist;
    DevBuf *buf;
};

// the encoder's passes over rows [n, dim] with the m codeword indexes given; enqueued on st.  With res, chunk by chunk
// rows - cent[lists] goes into res->buf (one chunk of whole rows, so the scratch stays bounded) and the chunk's residuals are encoded.
int pq_encode_chunks(const std::vector<mirx_index *> &cbidx, int dim, int m, const float *drows, int64_t n, uint8_t *codes,
                     DevBuf &sub, DevBuf &found, DevBuf &fval, const PqResidual *res, hipStream_t st) {
    const int dsub = dim / m;
    const int64_t chunk = std::min<int64_t>(n, PQ_ENCODE_CHUNK);
    if (res && res->buf->ensure((size_t)chunk * dim * sizeof(float)) != hipSuccess)
        return fail(MIRX_ENOMEM, "pq_encode: no memory for the residuals");
    if (sub.ensure((size_t)chunk * dsub * sizeof(float)) != hipSuccess || found.ensure((size_t)chunk * sizeof(int64_t)) != hipSuccess ||
        fval.ensure((size_t)chunk * sizeof(float)) != hipSuccess)
        return fail(MIRX_ENOMEM, "pq_encode: no memory for the encoder's scratch");
    for (int64_t c0 = 0; c0 < n; c0 += chunk) {
        const int64_t nc = std::min(chunk, n - c0);
        const float *src = drows + c0 * dim;
        if (res) {
            MIRX_HIP(launch_pq_residual(src, nc, dim, 0, dim, res->lists + c0, res->cent, res->nlist, res->buf->as<float>(), dim, st));
            src = res->buf->as<float>();
        }
        for (int j = 0; j < m; ++j) {
            MIRX_HIP(launch_ivf_place(src + (int64_t)j * dsub, nc, dim, dsub, nullptr, nullptr, sub.as<float>(), dsub, st));
            if (int rc = mirx_index_search(cbidx[(size_t)j], sub.as<float>(), nc, 1, nullptr, fval.as<float>(), found.as<int64_t>(), st))
                return rc;
            MIRX_HIP(launch_pq_pack(found.as<int64_t>(), nc, m, j, codes + c0 * m, st));
        }
    }
    return MIRX_OK;
}

// codes [n, m] (device) of rows [n, dim] (device) under cb (device [m][256][dim / m]): sub-vector j of every row searched in a flat
// index over sub-space j's codewords.  The m indexes live for the call only -- their search workspaces (tens of MB each) would
// outweigh the codes if the handle kept them.  Waits for its work, on failure too: the indexes are freed behind it.
// res (or null): the rows are coded by residual.
int pq_encode_rows(int device, int dim, int m, const float *cb, const float *drows, int64_t n, uint8_t *codes, DevBuf &sub,
                   DevBuf &found, DevBuf &fval, const PqResidual *res, hipStream_t st) {
    if (n == 0) return MIRX_OK;
    std::vector<mirx_index *> cbidx;
    if (int rc = build_codeword_indexes(dim, m, device, cb, cbidx)) return rc;
    const int rc = pq_encode_chunks(cbidx, dim, m, drows, n, codes, sub, found, fval, res, st);
    const hipError_t e = hipStreamSynchronize(st);
    free_codeword_indexes(cbidx);
    if (res) res->buf->release();                            // a chunk of whole fp32 rows (256 MiB at dim 1024): not worth holding
    if (rc) return rc;
    MIRX_HIP(e);
    return MIRX_OK;
}

// The one layout change behind add / remove / re-assign.  old_dst[p] = where resident row p goes (-1: dropped); the n_new rows of
// new_rows (device, [n_new, dim]) with new_ids go to new_dst.  total = the rows afterwards, new_off their offsets; seq / ids
// mirrors follow.  Everything is allocated before a row moves: MIRX_ENOMEM leaves the ivf untouched.
int relayout(mirx_ivf *ivf, const std::vector<int64_t> &old_dst, const void *new_rows, int64_t n_new,
             const std::vector<int64_t> &new_ids, const std::vector<int64_t> &new_dst, int64_t total,
             const std::vector<int64_t> &new_off, hipStream_t st, const double *new_norms = nullptr) {
    const int64_t n_old = ivf->size;
    DevBuf rows2, ids2, norms2;                                  // norms2: N2 travels with the ids (residual PQ under L2), 8 bytes a row
    const bool nrm = ivf->res_l2();
    const size_t pos_bytes = (size_t)std::max<int64_t>(n_old, n_new) * sizeof(int64_t);
    if (rows2.ensure((size_t)std::max<int64_t>(total, 1) * ivf->row_bytes()) != hipSuccess ||
        ids2.ensure((size_t)std::max<int64_t>(total, 1) * sizeof(int64_t)) != hipSuccess ||
        (nrm && norms2.ensure((size_t)std::max<int64_t>(total, 1) * sizeof(double)) != hipSuccess) ||
        ivf->pos.ensure(std::max<size_t>(pos_bytes, 8)) != hipSuccess ||
        ivf->newids.ensure((size_t)std::max<int64_t>(n_new, 1) * sizeof(int64_t)) != hipSuccess ||
        ivf->offsets.ensure((size_t)(ivf->nlist + 1) * sizeof(int64_t)) != hipSuccess)
        return fail(MIRX_ENOMEM, "ivf: no memory for the new layout");
    std::vector<int64_t> ids_h((size_t)total), seq_h((size_t)total);
    if (n_old) {
        MIRX_HIP(hipMemcpyAsync(ivf->pos.p, old_dst.data(), (size_t)n_old * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (ivf->sq8() || ivf->pq())
            MIRX_HIP(launch_ivf_place_codes(ivf->rows.as<uint8_t>(), n_old, ivf->code_ld(), ivf->pos.as<int64_t>(), rows2.as<uint8_t>(), st));
        else
            MIRX_HIP(launch_ivf_place(ivf->rows.as<float>(), n_old, ivf->dimp, ivf->dimp, nullptr, ivf->pos.as<int64_t>(),
                                      rows2.as<float>(), ivf->dimp, st));
        MIRX_HIP(launch_ivf_place_ids(ivf->ids.as<int64_t>(), n_old, ivf->pos.as<int64_t>(), ids2.as<int64_t>(), st));
        if (nrm) MIRX_HIP(launch_ivf_place_ids(ivf->norms.as<int64_t>(), n_old, ivf->pos.as<int64_t>(), norms2.as<int64_t>(), st));
        MIRX_HIP(hipStreamSynchronize(st));                     // pos is reused below
        for (int64_t p = 0; p < n_old; ++p)
            if (old_dst[(size_t)p] >= 0) {
                ids_h[(size_t)old_dst[(size_t)p]] = ivf->ids_h[(size_t)p];
                seq_h[(size_t)old_dst[(size_t)p]] = ivf->seq_h[(size_t)p];
            }
    }
    if (n_new) {
        MIRX_HIP(hipMemcpyAsync(ivf->pos.p, new_dst.data(), (size_t)n_new * sizeof(int64_t), hipMemcpyHostToDevice, st));
        MIRX_HIP(hipMemcpyAsync(ivf->newids.p, new_ids.data(), (size_t)n_new * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (ivf->pq())                                           // new_rows are the new rows' codes [n_new, m] (mirx_ivf_add)
            MIRX_HIP(launch_ivf_place_codes(static_cast<const uint8_t *>(new_rows), n_new, ivf->pq_m, ivf->pos.as<int64_t>(),
                                            rows2.as<uint8_t>(), st));
        else if (ivf->sq8())
            MIRX_HIP(launch_sq8_encode_place(static_cast<const float *>(new_rows), n_new, ivf->dim, ivf->vmin(), ivf->scale(),
                                             ivf->pos.as<int64_t>(), rows2.as<uint8_t>(), ivf->dimp, st));
        else
            MIRX_HIP(launch_ivf_place(static_cast<const float *>(new_rows), n_new, ivf->dim, ivf->dim, nullptr,
                                      ivf->pos.as<int64_t>(), rows2.as<float>(), ivf->dimp, st));
        MIRX_HIP(launch_ivf_place_ids(ivf->newids.as<int64_t>(), n_new, ivf->pos.as<int64_t>(), ids2.as<int64_t>(), st));
        if (nrm)
            MIRX_HIP(launch_ivf_place_ids(reinterpret_cast<const int64_t *>(new_norms), n_new, ivf->pos.as<int64_t>(),
                                          norms2.as<int64_t>(), st));
        for (int64_t j = 0; j < n_new; ++j) {
            ids_h[(size_t)new_dst[(size_t)j]] = new_ids[(size_t)j];
            seq_h[(size_t)new_dst[(size_t)j]] = ivf->next_seq + j;
        }
        ivf->next_seq += n_new;
    }
    MIRX_HIP(hipMemcpyAsync(ivf->offsets.p, new_off.data(), (size_t)(ivf->nlist + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    MIRX_HIP(hipStreamSynchronize(st));
    std::swap(ivf->rows.p, rows2.p);
    std::swap(ivf->rows.bytes, rows2.bytes);
    std::swap(ivf->ids.p, ids2.p);
    std::swap(ivf->ids.bytes, ids2.bytes);
    if (nrm) {
        std::swap(ivf->norms.p, norms2.p);
        std::swap(ivf->norms.bytes, norms2.bytes);
    }
    ivf->ids_h.swap(ids_h);
    ivf->seq_h.swap(seq_h);
    ivf->off_h = new_off;
    ivf->size = total;
    return MIRX_OK;
}

// the resident rows to the lists of the current centroids, insertion order kept inside each list (fp32 rows only: coded_rows_keep_trained_parts)
int reassign_resident(mirx_ivf *ivf, hipStream_t st) {
    const int64_t n = ivf->size;
    if (n == 0) return MIRX_OK;
    const float *flat = ivf->rows.as<float>();
    if (ivf->dimp != ivf->dim) {                                 // the centroid search reads rows of `dim` floats
        MIRX_HIP(ivf->stage.ensure((size_t)n * ivf->dim * sizeof(float)));
        MIRX_HIP(launch_ivf_place(ivf->rows.as<float>(), n, ivf->dimp, ivf->dim, nullptr, nullptr, ivf->stage.as<float>(), ivf->dim, st));
        flat = ivf->stage.as<float>();
    }
    std::vector<int64_t> lists;
    if (int rc = assign_to_host(ivf, flat, n, lists, st)) return rc;
    std::vector<int64_t> by_seq((size_t)n);
    std::iota(by_seq.begin(), by_seq.end(), (int64_t)0);
    std::sort(by_seq.begin(), by_seq.end(), [&](int64_t a, int64_t b) { return ivf->seq_h[(size_t)a] < ivf->seq_h[(size_t)b]; });
    std::vector<int64_t> off((size_t)ivf->nlist + 1, 0), dst((size_t)n);
    for (int64_t v : lists) ++off[(size_t)v + 1];
    for (int l = 0; l < ivf->nlist; ++l) off[(size_t)l + 1] += off[(size_t)l];
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (int64_t p : by_seq) dst[(size_t)p] = cur[(size_t)lists[(size_t)p]]++;
    const int64_t keep_seq = ivf->next_seq;
    const int rc = relayout(ivf, dst, nullptr, 0, {}, {}, n, off, st);
    ivf->next_seq = keep_seq;
    return rc;
}

int fix_centroids(mirx_ivf *ivf, hipStream_t st) {
    if (int rc = rebuild_centroid_index(ivf)) return rc;
    return reassign_resident(ivf, st);
}

// ---- mirx_ivf_search's per-kind step: one internal batch's scores into ivf->scores, compact rows of ld doubles ------------------
// nb queries qb with their np nearest lists in ivf->pids (nearest first); out_probes (or null) receives the batch's probes
struct SearchBatch {
    const float *qb;
    int nb, np;
    int64_t ld;
    int32_t *out_probes;
};

// what one PQ query costs beside its compact row: its m x 2 KiB table, and with residual coding a base per probed list and QQ
int64_t pq_query_bytes(const mirx_ivf *ivf, int np) {
    return (int64_t)ivf->pq_m * 256 * sizeof(double) + (ivf->pq_res ? (int64_t)8 * np + 8 : 0);
}

hipError_t scan_workspace(mirx_ivf *ivf, int64_t per, int np) {
    const int nlist = ivf->nlist;
    hipError_t e;
    if ((e = ivf->q32p.ensure((size_t)per * ivf->dimp * sizeof(float))) != hipSuccess ||
        (e = ivf->cntcur.ensure((size_t)2 * nlist * sizeof(int))) != hipSuccess ||
        (e = ivf->pairoff.ensure((size_t)(nlist + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = ivf->itemoff.ensure((size_t)(nlist + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = ivf->pair_q.ensure((size_t)per * np * sizeof(int32_t))) != hipSuccess)
        return e;
    return ivf->pair_off.ensure((size_t)per * np * sizeof(int32_t));
}

hipError_t pq_workspace(mirx_ivf *ivf, int64_t per, int np) {
    hipError_t e;
    if (ivf->pq_res && ((e = ivf->pq_base.ensure((size_t)per * np * sizeof(double))) != hipSuccess ||
                        (e = ivf->pq_qq.ensure((size_t)per * sizeof(double))) != hipSuccess))
        return e;
    if ((e = ivf->tables.ensure((size_t)per * ivf->pq_m * 256 * sizeof(double))) != hipSuccess ||
        (e = ivf->cntcur.ensure((size_t)ivf->nlist * sizeof(int))) != hipSuccess)
        return e;
    return ivf->itemoff.ensure((size_t)(per + 1) * sizeof(int32_t));
}

// FLAT and SQ8: the padded queries, the probes inverted into per-list (query, offset) pairs, the rows of every probed list scored
int scan_scores(mirx_ivf *ivf, const SearchBatch &b, hipStream_t st) {
    const int nlist = ivf->nlist, dimp = ivf->dimp, qt = ivf_query_tile(dimp);
    MIRX_HIP(launch_ivf_place(b.qb, b.nb, ivf->dim, ivf->dim, nullptr, nullptr, ivf->q32p.as<float>(), dimp, st));
    MIRX_HIP(launch_ivf_invert(ivf->pids.as<int64_t>(), b.nb, b.np, ivf->offsets.as<int64_t>(), nlist, qt, ivf->probes.as<int32_t>(),
                               b.out_probes, ivf->qoff.as<int32_t>(), ivf->cntcur.as<int>(), ivf->pairoff.as<int32_t>(),
                               ivf->itemoff.as<int32_t>(), ivf->pair_q.as<int32_t>(), ivf->pair_off.as<int32_t>(), ivf->stats_dev, st));
    IvfScoreArgs sa{};
    sa.q32p = ivf->q32p.as<float>();
    sa.rows = ivf->rows.p;
    sa.vmin = ivf->sq8() ? ivf->vmin() : nullptr;
    sa.scale = ivf->sq8() ? ivf->scale() : nullptr;
    sa.dimp = dimp;
    sa.nlist = nlist;
    sa.qt = qt;
    sa.offsets = ivf->offsets.as<int64_t>();
    sa.pairoff = ivf->pairoff.as<int32_t>();
    sa.itemoff = ivf->itemoff.as<int32_t>();
    sa.pair_q = ivf->pair_q.as<int32_t>();
    sa.pair_off = ivf->pair_off.as<int32_t>();
    sa.out = ivf->scores.as<double>();
    sa.ld = b.ld;
    MIRX_HIP(launch_ivf_scores(sa, ivf->metric, st));
    return MIRX_OK;
}

// PQ: the probes, every query's tables (residual: and its bases), the items of the scan, the ADC scan
int pq_scores(mirx_ivf *ivf, const SearchBatch &b, hipStream_t st) {
    const int nlist = ivf->nlist, m = ivf->pq_m;
    const bool res = ivf->pq_res, res_l2 = ivf->res_l2();
    MIRX_HIP(launch_ivf_probes(ivf->pids.as<int64_t>(), b.nb, b.np, ivf->offsets.as<int64_t>(), nlist, ivf->probes.as<int32_t>(),
                               b.out_probes, ivf->qoff.as<int32_t>(), ivf->cntcur.as<int>(), st));
    MIRX_HIP(launch_pq_tables(b.qb, b.nb, ivf->dim, m, res ? MIRX_METRIC_IP : ivf->metric, ivf->codebooks.as<float>(),
                              ivf->tables.as<double>(), st));
    if (res)
        MIRX_HIP(launch_pq_base(b.qb, b.nb, ivf->dim, m, ivf->probes.as<int32_t>(), b.np, ivf->centroids.as<float>(), nlist,
                                ivf->pq_base.as<double>(), res_l2 ? ivf->pq_qq.as<double>() : nullptr, st));
    MIRX_HIP(launch_pq_items(ivf->qoff.as<int32_t>(), b.nb, b.np, ivf->cntcur.as<int>(), nlist, ivf->itemoff.as<int32_t>(),
                             ivf->stats_dev, st));
    PqScanArgs sa{};
    sa.tables = ivf->tables.as<double>();
    sa.codes = ivf->rows.as<uint8_t>();
    sa.m = m;
    sa.nq = b.nb;
    sa.nprobe = b.np;
    sa.probes = ivf->probes.as<int32_t>();
    sa.qoff = ivf->qoff.as<int32_t>();
    sa.offsets = ivf->offsets.as<int64_t>();
    sa.itemoff = ivf->itemoff.as<int32_t>();
    sa.out = ivf->scores.as<double>();
    sa.ld = b.ld;
    sa.base = res ? ivf->pq_base.as<double>() : nullptr;
    sa.qq = res_l2 ? ivf->pq_qq.as<double>() : nullptr;
    sa.n2 = res_l2 ? ivf->norms.as<double>() : nullptr;
    MIRX_HIP(launch_pq_scan(sa, ivf->metric, st));
    return MIRX_OK;
}

}  // namespace

extern "C" {

static int create_ivf(int dim, int metric, int nlist, int kind, int m, bool by_residual, int device, mirx_ivf **out);   // behind every create call

int mirx_ivf_query_tile(int dim) {
    if (dim < 1 || dim > MIRX_IVF_MAX_DIM) return -1;
    return ivf_query_tile((int)round_up(dim, DIM_ALIGN));
}
int mirx_ivf_row_block(void) { return IVF_ROWS; }

int mirx_ivf_create(int dim, int metric, int nlist, int device, mirx_ivf **out) {
    return mirx_ivf_create_typed(dim, metric, nlist, MIRX_IVF_FLAT, device, out);
}

int mirx_ivf_create_typed(int dim, int metric, int nlist, int kind, int device, mirx_ivf **out) {
    MIRX_CHECK(out, "ivf_create: out is null");
    *out = nullptr;
    MIRX_CHECK(kind == MIRX_IVF_FLAT || kind == MIRX_IVF_SQ8,
               "ivf_create: unknown kind (MIRX_IVF_FLAT, MIRX_IVF_SQ8; MIRX_IVF_PQ needs m: mirx_ivf_create_pq)");
    return create_ivf(dim, metric, nlist, kind, 0, false, device, out);
}

int mirx_ivf_create_pq(int dim, int metric, int nlist, int m, int nbits, int device, mirx_ivf **out) {
    MIRX_CHECK(out, "ivf_create_pq: out is null");
    return mirx_ivf_create_pq_ex(dim, metric, nlist, m, nbits, 0, device, out);
}

int mirx_ivf_create_pq_ex(int dim, int metric, int nlist, int m, int nbits, int by_residual, int device, mirx_ivf **out) {
    MIRX_CHECK(out, "ivf_create_pq_ex: out is null");
    *out = nullptr;
    MIRX_CHECK(by_residual == 0 || by_residual == 1, "ivf_create_pq_ex: by_residual must be 0 or 1");
    MIRX_CHECK(nbits == 8, "ivf_create_pq: nbits must be 8 (256 codewords per sub-quantiser)");
    MIRX_CHECK(m >= 4 && m <= PQ_MAX_M && m % 4 == 0, "ivf_create_pq: m must be a multiple of 4 in 4 .. 64");
    MIRX_CHECK(dim >= 1 && dim % (4 * m) == 0, "ivf_create_pq: dim must be a multiple of 4 m");
    return create_ivf(dim, metric, nlist, MIRX_IVF_PQ, m, by_residual == 1, device, out);
}

int mirx_ivf_pq_m(const mirx_ivf *ivf) { return ivf && ivf->pq() ? ivf->pq_m : -1; }
int mirx_ivf_pq_by_residual(const mirx_ivf *ivf) { return ivf && ivf->pq() ? (ivf->pq_res ? 1 : 0) : -1; }
int mirx_ivf_pq_item_rows(void) { return PQ_ITEM_ROWS; }

static int create_ivf(int dim, int metric, int nlist, int kind, int m, bool by_residual, int device, mirx_ivf **out) {
    MIRX_CHECK(dim >= 1 && dim <= MIRX_IVF_MAX_DIM, "ivf_create: dim out of range (1 .. 2048)");
    MIRX_CHECK(metric == MIRX_METRIC_IP || metric == MIRX_METRIC_NEG_L2, "ivf_create: unknown metric");
    MIRX_CHECK(nlist >= 1 && nlist <= MIRX_IVF_MAX_NLIST, "ivf_create: nlist out of range (1 .. 65536)");
    int ndev = 0;
    MIRX_HIP(hipGetDeviceCount(&ndev));
    MIRX_CHECK(device >= 0 && device < ndev, "ivf_create: no such device");
    DeviceGuard dg(device);
    if (!dg.ok) return fail(MIRX_EHIP, "ivf_create: cannot select device");
    mirx_ivf *ivf = new (std::nothrow) mirx_ivf();
    if (!ivf) return fail(MIRX_ENOMEM, "ivf_create: host allocation failed");
    ivf->dim = dim;
    ivf->dimp = (int)round_up(dim, DIM_ALIGN);
    ivf->metric = metric;
    ivf->nlist = nlist;
    ivf->device = device;
    ivf->kind = kind;
    ivf->pq_m = m;
    ivf->pq_res = by_residual;
    ivf->off_h.assign((size_t)nlist + 1, 0);
    hipError_t e;
    if ((e = ivf->centroids.ensure((size_t)nlist * dim * sizeof(float))) != hipSuccess ||
        (e = ivf->offsets.ensure((size_t)(nlist + 1) * sizeof(int64_t))) != hipSuccess ||
        (e = hipMemset(ivf->offsets.p, 0, (size_t)(nlist + 1) * sizeof(int64_t))) != hipSuccess ||
        (kind == MIRX_IVF_SQ8 && (e = ivf->range.ensure((size_t)2 * ivf->dimp * sizeof(float))) != hipSuccess) ||
        (kind == MIRX_IVF_PQ && (e = ivf->codebooks.ensure((size_t)256 * dim * sizeof(float))) != hipSuccess) ||
        (e = hipMalloc(&ivf->stats_dev, 3 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(ivf->stats_dev, 0, 3 * sizeof(unsigned long long))) != hipSuccess) {
        mirx_ivf_destroy(ivf);
        return fail(MIRX_ENOMEM, std::string("ivf_create: ") + hipGetErrorString(e));
    }
    *out = ivf;
    return MIRX_OK;
}

int mirx_ivf_kind(const mirx_ivf *ivf) { return ivf ? ivf->kind : -1; }

void mirx_ivf_destroy(mirx_ivf *ivf) {
    if (!ivf) return;
    DeviceGuard dg(ivf->device);
    if (ivf->cent) mirx_index_destroy(ivf->cent);
    if (ivf->stats_dev) (void)hipFree(ivf->stats_dev);
    delete ivf;                           // every DevBuf releases itself, inside dg's scope
}

int mirx_ivf_train(mirx_ivf *ivf, const float *rows, int64_t n, const int64_t *init_positions_or_null, int iters, void *stream) {
    MIRX_CHECK(ivf && rows, "ivf_train: null argument");
    MIRX_CHECK(n >= ivf->nlist, "ivf_train: fewer rows than lists");
    MIRX_CHECK(n <= 0x7FFFFF00ll, "ivf_train: more than 2^31 rows");
    MIRX_CHECK(iters >= 0, "ivf_train: iters must not be negative");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_train")) return rc;
    const int nlist = ivf->nlist, dim = ivf->dim;
    std::vector<int64_t> start((size_t)nlist);
    for (int j = 0; j < nlist; ++j) {
        start[(size_t)j] = init_positions_or_null ? init_positions_or_null[j] : (int64_t)j * n / nlist;
        MIRX_CHECK(start[(size_t)j] >= 0 && start[(size_t)j] < n, "ivf_train: an initial position is not a row");
    }
    MIRX_IVF_ENTER(ivf, "ivf_train");
    hipStream_t st = (hipStream_t)stream;
    const float *drows = nullptr;
    DevBuf trows;                                      // a host caller's rows for the length of the call (the stage serves the re-assignment)
    if (int rc = device_rows(ivf, rows, n, trows, &drows)) return rc;
    if (int rc = lloyd(ivf, drows, n, dim, ivf->metric, nlist, start, iters, ivf->centroids.as<float>(), st)) {
        // the centroid array is partly trained: as before the loop moved into lloyd(), the index over the centroids follows it
        // (the resident rows keep their lists; the next train / set_centroids re-assigns them)
        (void)hipStreamSynchronize(st);
        (void)rebuild_centroid_index(ivf);
        return rc;
    }
    return fix_centroids(ivf, st);
}

int mirx_ivf_set_centroids(mirx_ivf *ivf, const float *centroids) {
    MIRX_CHECK(ivf && centroids, "ivf_set_centroids: null argument");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_set_centroids")) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_set_centroids");
    MIRX_HIP(hipMemcpy(ivf->centroids.p, centroids, (size_t)ivf->nlist * ivf->dim * sizeof(float), hipMemcpyDefault));
    return fix_centroids(ivf, nullptr);
}

int mirx_ivf_get_centroids(const mirx_ivf *ivf, float *out_centroids) {
    MIRX_CHECK(ivf && out_centroids, "ivf_get_centroids: null argument");
    if (int rc = trained_parts_fixed(ivf, "ivf_get_centroids", CENTROIDS)) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_get_centroids");
    MIRX_HIP(hipMemcpy(out_centroids, ivf->centroids.p, (size_t)ivf->nlist * ivf->dim * sizeof(float), hipMemcpyDefault));
    return MIRX_OK;
}

int mirx_ivf_add(mirx_ivf *ivf, const float *rows, int64_t n, const int64_t *ids_or_null) {
    MIRX_CHECK(ivf && n >= 0 && (rows || n == 0), "ivf_add: bad argument");
    if (int rc = trained_parts_fixed(ivf, "ivf_add", ALL_PARTS)) return rc;
    MIRX_CHECK(ivf->size + n <= 0x7FFFFF00ll, "ivf_add: more than 2^31 rows per index");
    MIRX_IVF_ENTER(ivf, "ivf_add");
    if (n == 0) return MIRX_OK;
    const float *drows = nullptr;
    if (int rc = device_rows(ivf, rows, n, ivf->stage, &drows)) return rc;
    std::vector<int64_t> lists, new_ids((size_t)n);
    if (int rc = assign_to_host(ivf, drows, n, lists, nullptr)) return rc;
    if (ids_or_null) {
        MIRX_HIP(hipMemcpy(new_ids.data(), ids_or_null, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
    } else {
        const int64_t first = std::max(ivf->next_auto, ivf->size);
        for (int64_t i = 0; i < n; ++i) new_ids[(size_t)i] = first + i;
        ivf->next_auto = first + n;
    }
    const int nlist = ivf->nlist;
    std::vector<int64_t> add((size_t)nlist + 1, 0), off((size_t)nlist + 1, 0);
    for (int64_t v : lists) ++add[(size_t)v + 1];
    for (int l = 0; l < nlist; ++l) add[(size_t)l + 1] += add[(size_t)l];          // new rows in front of list l
    for (int l = 0; l <= nlist; ++l) off[(size_t)l] = ivf->off_h[(size_t)l] + add[(size_t)l];
    std::vector<int64_t> old_dst((size_t)ivf->size), new_dst((size_t)n), at((size_t)nlist);
    for (int l = 0; l < nlist; ++l) {
        for (int64_t p = ivf->off_h[(size_t)l]; p < ivf->off_h[(size_t)l + 1]; ++p) old_dst[(size_t)p] = p + add[(size_t)l];
        at[(size_t)l] = ivf->off_h[(size_t)l + 1] + add[(size_t)l];                // behind the list's resident rows
    }
    for (int64_t j = 0; j < n; ++j) new_dst[(size_t)j] = at[(size_t)lists[(size_t)j]]++;
    const void *placed = drows;
    if (ivf->pq()) {                                             // the list came from the original row; now the row becomes its codes
        if (ivf->pq_codes.ensure((size_t)n * ivf->pq_m) != hipSuccess) return fail(MIRX_ENOMEM, "ivf_add: no memory for the new codes");
        if (ivf->pq_res) {                                       // the new rows' lists on the device: their centroids are subtracted
            if (ivf->pq_lists.ensure((size_t)n * sizeof(int64_t)) != hipSuccess ||
                (ivf->res_l2() && ivf->pq_n2.ensure((size_t)n * sizeof(double)) != hipSuccess))
                return fail(MIRX_ENOMEM, "ivf_add: no memory for the new rows' lists and norms");
            MIRX_HIP(hipMemcpy(ivf->pq_lists.p, lists.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        const PqResidual res{ivf->pq_lists.as<int64_t>(), ivf->centroids.as<float>(), nlist, &ivf->pq_resid};
        if (int rc = pq_encode_rows(ivf->device, ivf->dim, ivf->pq_m, ivf->codebooks.as<float>(), drows, n,
                                    ivf->pq_codes.as<uint8_t>(), ivf->pq_sub, ivf->pq_found, ivf->fval, ivf->pq_res ? &res : nullptr,
                                    nullptr))
            return rc;
        if (ivf->res_l2())
            MIRX_HIP(launch_pq_norms(ivf->pq_codes.as<uint8_t>(), n, ivf->dim, ivf->pq_m, res.lists, ivf->centroids.as<float>(), nlist,
                                     ivf->codebooks.as<float>(), ivf->pq_n2.as<double>(), nullptr));
        placed = ivf->pq_codes.p;
    }
    return relayout(ivf, old_dst, placed, n, new_ids, new_dst, ivf->size + n, off, nullptr,
                    ivf->res_l2() ? ivf->pq_n2.as<double>() : nullptr);
}

int mirx_ivf_remove_ids(mirx_ivf *ivf, const int64_t *ids, int64_t n, int64_t *out_removed_or_null, void *stream) {
    MIRX_CHECK(ivf && n >= 0 && (ids || n == 0), "ivf_remove_ids: bad argument");
    MIRX_IVF_ENTER(ivf, "ivf_remove_ids");
    if (out_removed_or_null) *out_removed_or_null = 0;
    if (n == 0 || ivf->size == 0) return MIRX_OK;
    std::vector<int64_t> req((size_t)n);
    MIRX_HIP(hipMemcpy(req.data(), ids, (size_t)n * sizeof(int64_t), hipMemcpyDefault));
    const std::unordered_set<int64_t> gone(req.begin(), req.end());
    const int nlist = ivf->nlist;
    std::vector<int64_t> dst((size_t)ivf->size), off((size_t)nlist + 1, 0);
    int64_t kept = 0;
    for (int l = 0; l < nlist; ++l) {
        off[(size_t)l] = kept;
        for (int64_t p = ivf->off_h[(size_t)l]; p < ivf->off_h[(size_t)l + 1]; ++p)
            dst[(size_t)p] = gone.count(ivf->ids_h[(size_t)p]) ? -1 : kept++;
    }
    off[(size_t)nlist] = kept;
    const int64_t removed = ivf->size - kept;
    if (removed) {
        if (int rc = relayout(ivf, dst, nullptr, 0, {}, {}, kept, off, (hipStream_t)stream)) return rc;
    }
    if (out_removed_or_null) *out_removed_or_null = removed;
    return MIRX_OK;
}

int64_t mirx_ivf_size(const mirx_ivf *ivf) { return ivf ? ivf->size : -1; }

int mirx_ivf_sq8_train(mirx_ivf *ivf, const float *rows, int64_t n, void *stream) {
    MIRX_CHECK(ivf && rows, "ivf_sq8_train: null argument");
    MIRX_IVF_SQ8_ONLY(ivf, "ivf_sq8_train");
    MIRX_CHECK(n >= 1, "ivf_sq8_train: no rows");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_sq8_train")) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_sq8_train");
    hipStream_t st = (hipStream_t)stream;
    const float *drows = nullptr;
    DevBuf trows;
    if (int rc = device_rows(ivf, rows, n, trows, &drows)) return rc;
    MIRX_HIP(ivf->upd.ensure((size_t)sq8_minmax_parts(n) * 2 * ivf->dim * sizeof(float)));
    MIRX_HIP(launch_sq8_range(drows, n, ivf->dim, ivf->dimp, ivf->upd.as<float>(), ivf->range.as<float>(),
                              ivf->range.as<float>() + ivf->dimp, st));
    MIRX_HIP(hipStreamSynchronize(st));                      // trows may be a copy that ends with the call
    ivf->range_fixed = true;
    return MIRX_OK;
}

int mirx_ivf_sq8_set_range(mirx_ivf *ivf, const float *vmin, const float *scale) {
    MIRX_CHECK(ivf && vmin && scale, "ivf_sq8_set_range: null argument");
    MIRX_IVF_SQ8_ONLY(ivf, "ivf_sq8_set_range");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_sq8_set_range")) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_sq8_set_range");
    MIRX_HIP(hipMemset(ivf->range.p, 0, (size_t)2 * ivf->dimp * sizeof(float)));
    MIRX_HIP(hipMemcpy(ivf->range.p, vmin, (size_t)ivf->dim * sizeof(float), hipMemcpyDefault));
    MIRX_HIP(hipMemcpy(ivf->range.as<float>() + ivf->dimp, scale, (size_t)ivf->dim * sizeof(float), hipMemcpyDefault));
    ivf->range_fixed = true;
    return MIRX_OK;
}

int mirx_ivf_sq8_get_range(const mirx_ivf *ivf, float *out_vmin, float *out_scale) {
    MIRX_CHECK(ivf && out_vmin && out_scale, "ivf_sq8_get_range: null argument");
    MIRX_IVF_SQ8_ONLY(ivf, "ivf_sq8_get_range");
    if (int rc = trained_parts_fixed(ivf, "ivf_sq8_get_range", RANGE)) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_sq8_get_range");
    MIRX_HIP(hipMemcpy(out_vmin, ivf->vmin(), (size_t)ivf->dim * sizeof(float), hipMemcpyDefault));
    MIRX_HIP(hipMemcpy(out_scale, ivf->scale(), (size_t)ivf->dim * sizeof(float), hipMemcpyDefault));
    return MIRX_OK;
}

// ids and list numbers of the resident rows in list-major order, to device arrays (either may be null)
static int resident_ids_lists(const mirx_ivf *ivf, int64_t *out_ids, int64_t *out_lists) {
    if (out_ids) MIRX_HIP(hipMemcpy(out_ids, ivf->ids.p, (size_t)ivf->size * sizeof(int64_t), hipMemcpyDeviceToDevice));
    if (out_lists) {
        std::vector<int64_t> lists((size_t)ivf->size);
        for (int l = 0; l < ivf->nlist; ++l)
            std::fill(lists.begin() + ivf->off_h[(size_t)l], lists.begin() + ivf->off_h[(size_t)l + 1], (int64_t)l);
        MIRX_HIP(hipMemcpy(out_lists, lists.data(), (size_t)ivf->size * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    return MIRX_OK;
}

int mirx_ivf_get_codes(const mirx_ivf *ivf, uint8_t *out_codes, int64_t *out_ids_or_null, int64_t *out_lists_or_null) {
    MIRX_CHECK(ivf && (out_codes || ivf->size == 0), "ivf_get_codes: null argument");
    MIRX_IVF_CODED_ONLY(ivf, "ivf_get_codes");
    MIRX_IVF_ENTER(ivf, "ivf_get_codes");
    if (ivf->size == 0) return MIRX_OK;
    const size_t width = ivf->pq() ? (size_t)ivf->pq_m : (size_t)ivf->dim;         // the codes of a row, without SQ8's padding
    MIRX_HIP(hipMemcpy2D(out_codes, width, ivf->rows.p, (size_t)ivf->code_ld(), width, (size_t)ivf->size, hipMemcpyDeviceToDevice));
    return resident_ids_lists(ivf, out_ids_or_null, out_lists_or_null);
}

int mirx_ivf_reconstruct(const mirx_ivf *ivf, float *out_rows, int64_t *out_ids_or_null) {
    MIRX_CHECK(ivf && (out_rows || ivf->size == 0), "ivf_reconstruct: null argument");
    MIRX_IVF_CODED_ONLY(ivf, "ivf_reconstruct");
    MIRX_IVF_ENTER(ivf, "ivf_reconstruct");
    if (ivf->size == 0) return MIRX_OK;
    DevBuf dlists;                                           // residual PQ: every row's list, for its centroid
    if (ivf->pq() && ivf->pq_res) {
        if (dlists.ensure((size_t)ivf->size * sizeof(int64_t)) != hipSuccess) return fail(MIRX_ENOMEM, "ivf_reconstruct: no memory for the lists");
        if (int rc = resident_ids_lists(ivf, nullptr, dlists.as<int64_t>())) return rc;
        MIRX_HIP(launch_pq_decode_residual(ivf->rows.as<uint8_t>(), ivf->size, ivf->dim, ivf->pq_m, ivf->codebooks.as<float>(),
                                           dlists.as<int64_t>(), ivf->centroids.as<float>(), ivf->nlist, out_rows, nullptr));
    } else if (ivf->pq())
        MIRX_HIP(launch_pq_decode(ivf->rows.as<uint8_t>(), ivf->size, ivf->dim, ivf->pq_m, ivf->codebooks.as<float>(), out_rows, nullptr));
    else
        MIRX_HIP(launch_sq8_decode(ivf->rows.as<uint8_t>(), ivf->size, ivf->dimp, ivf->dim, ivf->vmin(), ivf->scale(), out_rows, nullptr));
    MIRX_HIP(hipStreamSynchronize(nullptr));
    return resident_ids_lists(ivf, out_ids_or_null, nullptr);
}

int mirx_sq8_encode(const float *rows, int64_t n, int dim, const float *vmin, const float *scale, uint8_t *out_codes, void *stream) {
    MIRX_CHECK(n >= 0 && dim >= 1 && dim <= MIRX_IVF_MAX_DIM, "sq8_encode: n or dim out of range");
    MIRX_CHECK((rows && out_codes && vmin && scale) || n == 0, "sq8_encode: null argument");
    if (n == 0) return MIRX_OK;
    hipStream_t st = (hipStream_t)stream;
    const int dimp = (int)round_up(dim, DIM_ALIGN);
    DevBuf padded;                                           // the kernel stores whole words: rows of dimp bytes, copied out below
    if (padded.ensure((size_t)n * dimp) != hipSuccess) return fail(MIRX_ENOMEM, "sq8_encode: no memory for the padded codes");
    MIRX_HIP(launch_sq8_encode_place(rows, n, dim, vmin, scale, nullptr, padded.as<uint8_t>(), dimp, st));
    MIRX_HIP(hipMemcpy2DAsync(out_codes, (size_t)dim, padded.p, (size_t)dimp, (size_t)dim, (size_t)n, hipMemcpyDeviceToDevice, st));
    MIRX_HIP(hipStreamSynchronize(st));
    return MIRX_OK;
}

int mirx_sq8_decode(const uint8_t *codes, int64_t n, int dim, const float *vmin, const float *scale, float *out_rows, void *stream) {
    MIRX_CHECK(n >= 0 && dim >= 1 && dim <= MIRX_IVF_MAX_DIM, "sq8_decode: n or dim out of range");
    MIRX_CHECK((codes && out_rows && vmin && scale) || n == 0, "sq8_decode: null argument");
    MIRX_HIP(launch_sq8_decode(codes, n, dim, dim, vmin, scale, out_rows, (hipStream_t)stream));
    return MIRX_OK;
}

int mirx_ivf_pq_train(mirx_ivf *ivf, const float *rows, int64_t n, int iters, void *stream) {
    MIRX_CHECK(ivf && rows, "ivf_pq_train: null argument");
    MIRX_IVF_PQ_ONLY(ivf, "ivf_pq_train");
    MIRX_CHECK(n >= 256, "ivf_pq_train: fewer rows than codewords (256)");
    MIRX_CHECK(n <= 0x7FFFFF00ll, "ivf_pq_train: more than 2^31 rows");
    MIRX_CHECK(iters >= 0, "ivf_pq_train: iters must not be negative");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_pq_train")) return rc;
    if (ivf->pq_res && !ivf->cent)
        return fail(MIRX_ESTATE, "ivf_pq_train: residual coding trains on rows minus their centroids, and the centroids are not "
                                 "fixed yet (mirx_ivf_train / _set_centroids)");
    MIRX_IVF_ENTER(ivf, "ivf_pq_train");
    hipStream_t st = (hipStream_t)stream;
    const float *drows = nullptr;
    DevBuf trows;
    if (int rc = device_rows(ivf, rows, n, trows, &drows)) return rc;
    const int m = ivf->pq_m, dsub = ivf->dim / m;
    if (ivf->pq_res) {                                       // the training rows' lists; lloyd() below reuses ivf->lists
        std::vector<int64_t> lists;
        if (int rc = assign_to_host(ivf, drows, n, lists, st)) return rc;
        MIRX_HIP(ivf->pq_lists.ensure((size_t)n * sizeof(int64_t)));
        MIRX_HIP(hipMemcpyAsync(ivf->pq_lists.p, ivf->lists.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    std::vector<int64_t> start(256);
    for (int c = 0; c < 256; ++c) start[(size_t)c] = (int64_t)c * n / 256;
    MIRX_HIP(ivf->pq_sub.ensure((size_t)n * dsub * sizeof(float)));
    ivf->cb_fixed = false;                                   // not fixed while they are trained
    for (int j = 0; j < m; ++j) {                            // mirx_ivf_train's loop on the columns of sub-space j, 256 lists, always L2
        if (ivf->pq_res)                                     // sub-space j of row - centroid, straight into the trainer's buffer
            MIRX_HIP(launch_pq_residual(drows, n, ivf->dim, j * dsub, dsub, ivf->pq_lists.as<int64_t>(), ivf->centroids.as<float>(),
                                        ivf->nlist, ivf->pq_sub.as<float>(), dsub, st));
        else
            MIRX_HIP(launch_ivf_place(drows + (int64_t)j * dsub, n, ivf->dim, dsub, nullptr, nullptr, ivf->pq_sub.as<float>(), dsub, st));
        if (int rc = lloyd(ivf, ivf->pq_sub.as<float>(), n, dsub, MIRX_METRIC_NEG_L2, 256, start, iters,
                           ivf->codebooks.as<float>() + (size_t)j * 256 * dsub, st))
            return rc;
    }
    ivf->cb_fixed = true;
    return MIRX_OK;
}

int mirx_ivf_pq_set_codebooks(mirx_ivf *ivf, const float *codebooks) {
    MIRX_CHECK(ivf && codebooks, "ivf_pq_set_codebooks: null argument");
    MIRX_IVF_PQ_ONLY(ivf, "ivf_pq_set_codebooks");
    if (int rc = coded_rows_keep_trained_parts(ivf, "ivf_pq_set_codebooks")) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_pq_set_codebooks");
    MIRX_HIP(hipMemcpy(ivf->codebooks.p, codebooks, (size_t)256 * ivf->dim * sizeof(float), hipMemcpyDefault));
    ivf->cb_fixed = true;
    return MIRX_OK;
}

int mirx_ivf_pq_get_codebooks(const mirx_ivf *ivf, float *out_codebooks) {
    MIRX_CHECK(ivf && out_codebooks, "ivf_pq_get_codebooks: null argument");
    MIRX_IVF_PQ_ONLY(ivf, "ivf_pq_get_codebooks");
    if (int rc = trained_parts_fixed(ivf, "ivf_pq_get_codebooks", CODEBOOKS)) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_pq_get_codebooks");
    MIRX_HIP(hipMemcpy(out_codebooks, ivf->codebooks.p, (size_t)256 * ivf->dim * sizeof(float), hipMemcpyDefault));
    return MIRX_OK;
}

int mirx_pq_encode(const float *rows, int64_t n, int dim, int m, const float *codebooks, uint8_t *out_codes, void *stream) {
    MIRX_CHECK(n >= 0 && pq_shape_ok(dim, m), "pq_encode: n, dim or m out of range (m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0)");
    MIRX_CHECK((rows && out_codes && codebooks) || n == 0, "pq_encode: null argument");
    if (n == 0) return MIRX_OK;
    int device = 0;
    MIRX_HIP(hipGetDevice(&device));
    DevBuf sub, found, fval;
    return pq_encode_rows(device, dim, m, codebooks, rows, n, out_codes, sub, found, fval, nullptr, (hipStream_t)stream);
}

int mirx_pq_decode(const uint8_t *codes, int64_t n, int dim, int m, const float *codebooks, float *out_rows, void *stream) {
    MIRX_CHECK(n >= 0 && pq_shape_ok(dim, m), "pq_decode: n, dim or m out of range (m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0)");
    MIRX_CHECK((codes && out_rows && codebooks) || n == 0, "pq_decode: null argument");
    MIRX_HIP(launch_pq_decode(codes, n, dim, m, codebooks, out_rows, (hipStream_t)stream));
    return MIRX_OK;
}

int mirx_pq_tables(const float *q, int64_t nq, int dim, int m, int metric, const float *codebooks, double *out_tables_f64,
                   void *stream) {
    MIRX_CHECK(nq >= 0 && pq_shape_ok(dim, m), "pq_tables: nq, dim or m out of range (m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0)");
    MIRX_CHECK(metric == MIRX_METRIC_IP || metric == MIRX_METRIC_NEG_L2, "pq_tables: unknown metric");
    MIRX_CHECK((q && out_tables_f64 && codebooks) || nq == 0, "pq_tables: null argument");
    MIRX_HIP(launch_pq_tables(q, nq, dim, m, metric, codebooks, out_tables_f64, (hipStream_t)stream));
    return MIRX_OK;
}

int mirx_ivf_get_norms(const mirx_ivf *ivf, double *out_norms_f64) {
    MIRX_CHECK(ivf && (out_norms_f64 || ivf->size == 0), "ivf_get_norms: null argument");
    MIRX_CHECK(ivf->res_l2(), "ivf_get_norms: only a residual IVF_PQ handle under L2 keeps norms");
    MIRX_IVF_ENTER(ivf, "ivf_get_norms");
    if (ivf->size == 0) return MIRX_OK;
    MIRX_HIP(hipMemcpy(out_norms_f64, ivf->norms.p, (size_t)ivf->size * sizeof(double), hipMemcpyDefault));
    return MIRX_OK;
}

int mirx_pq_residuals(const float *rows, int64_t n, int dim, const int64_t *lists, const float *centroids, int nlist,
                      float *out_rows, void *stream) {
    MIRX_CHECK(n >= 0 && dim >= 1 && dim <= MIRX_IVF_MAX_DIM && nlist >= 1 && nlist <= MIRX_IVF_MAX_NLIST,
               "pq_residuals: n, dim or nlist out of range");
    MIRX_CHECK((rows && lists && centroids && out_rows) || n == 0, "pq_residuals: null argument");
    MIRX_HIP(launch_pq_residual(rows, n, dim, 0, dim, lists, centroids, nlist, out_rows, dim, (hipStream_t)stream));
    return MIRX_OK;
}

int mirx_pq_bases(const float *q, int64_t nq, int dim, int m, const int32_t *lists, int nprobe, const float *centroids, int nlist,
                  double *out_base_f64, double *out_qq_f64_or_null, void *stream) {
    MIRX_CHECK(nq >= 0 && pq_shape_ok(dim, m), "pq_bases: nq, dim or m out of range (m % 4 == 0, 4 <= m <= 64, dim % (4 m) == 0)");
    MIRX_CHECK(nprobe >= 1 && nlist >= 1 && nlist <= MIRX_IVF_MAX_NLIST, "pq_bases: nprobe or nlist out of range");
    MIRX_CHECK((q && lists && centroids && out_base_f64) || nq == 0, "pq_bases: null argument");
    MIRX_CHECK(((uintptr_t)centroids & 15) == 0, "pq_bases: centroids must be 16-byte aligned");
    MIRX_HIP(launch_pq_base(q, nq, dim, m, lists, nprobe, centroids, nlist, out_base_f64, out_qq_f64_or_null, (hipStream_t)stream));
    return MIRX_OK;
}

int mirx_ivf_list_sizes(const mirx_ivf *ivf, int64_t *out_sizes) {
    MIRX_CHECK(ivf && out_sizes, "ivf_list_sizes: null argument");
    for (int l = 0; l < ivf->nlist; ++l) out_sizes[l] = ivf->off_h[(size_t)l + 1] - ivf->off_h[(size_t)l];
    return MIRX_OK;
}

int mirx_ivf_assign(mirx_ivf *ivf, const float *rows, int64_t n, int64_t *out_lists, void *stream) {
    MIRX_CHECK(ivf && n >= 0 && ((rows && out_lists) || n == 0), "ivf_assign: bad argument");
    if (int rc = trained_parts_fixed(ivf, "ivf_assign", CENTROIDS)) return rc;
    MIRX_IVF_ENTER(ivf, "ivf_assign");
    return assign_rows(ivf, rows, n, out_lists, (hipStream_t)stream);
}

int mirx_ivf_set_option(mirx_ivf *ivf, int option, int64_t value) {
    MIRX_CHECK(ivf, "ivf_set_option: null ivf");
    MIRX_CHECK(option == MIRX_IVF_OPT_SCORE_BYTES, "ivf_set_option: unknown option");
    MIRX_CHECK(value >= 0, "ivf_set_option: score bytes must be 0 (default) or a byte count");
    ivf->score_bytes = value;
    return MIRX_OK;
}

int mirx_ivf_search(mirx_ivf *ivf, const float *q, int64_t nq, int k, int nprobe, const int64_t *exclude_ids_or_null,
                    float *out_values_or_null, double *out_f64_or_null, int64_t *out_ids, int32_t *out_probes_or_null,
                    void *stream) {
    MIRX_CHECK(ivf && nq >= 0 && ((q && out_ids) || nq == 0), "ivf_search: null argument");
    MIRX_CHECK(out_values_or_null || out_f64_or_null || nq == 0, "ivf_search: both score outputs are null");
    MIRX_CHECK(k >= 1 && k <= MAX_K, "ivf_search: k out of range (1 .. 1024)");
    MIRX_CHECK(nprobe >= 1, "ivf_search: nprobe must be at least 1");
    if (int rc = trained_parts_fixed(ivf, "ivf_search", CENTROIDS)) return rc;   // rows imply the range / codebooks (mirx_ivf_add)
    MIRX_IVF_ENTER(ivf, "ivf_search");
    hipStream_t st = (hipStream_t)stream;
    const int nlist = ivf->nlist, np = std::min(nprobe, nlist);
    const bool pq = ivf->pq();
    ivf->last_nq = nq;
    ivf->last_batches = 0;
    MIRX_HIP(hipMemsetAsync(ivf->stats_dev, 0, 3 * sizeof(unsigned long long), st));
    if (nq == 0) return MIRX_OK;
    // a compact row is never longer than the np largest lists together
    std::vector<int64_t> sizes((size_t)nlist);
    int64_t blocks = 0;
    for (int l = 0; l < nlist; ++l) {
        sizes[(size_t)l] = ivf->off_h[(size_t)l + 1] - ivf->off_h[(size_t)l];
        blocks += (sizes[(size_t)l] + IVF_ROWS - 1) / IVF_ROWS;
    }
    std::partial_sort(sizes.begin(), sizes.begin() + np, sizes.end(), std::greater<int64_t>());
    const int64_t ld = std::max<int64_t>(1, std::accumulate(sizes.begin(), sizes.begin() + np, (int64_t)0));
    // the queries of one internal batch: a query's compact row of doubles (PQ: and its tables and bases) out of the one workspace
    // budget, the (query, probe) pairs bounded, the kind's work items within an int
    const int64_t budget = ivf->score_bytes > 0 ? ivf->score_bytes : (int64_t)SCORE_WS_BYTES;
    int64_t per = std::max<int64_t>(1, std::min<int64_t>(nq, budget / (ld * 8 + (pq ? pq_query_bytes(ivf, np) : 0))));
    per = std::min(per, std::max<int64_t>(1, MAX_BATCH_PAIRS / np));
    if (pq) {
        per = std::min(per, std::max<int64_t>(1, 0x7FFFFFFFll / ((ld + PQ_ITEM_ROWS - 1) / PQ_ITEM_ROWS)));
    } else {
        const int qt = ivf_query_tile(ivf->dimp);
        while (per > 1 && (per / qt + 1) * std::max<int64_t>(blocks, 1) > 0x7FFFFFFFll) per /= 2;
        MIRX_CHECK((per / qt + 1) * std::max<int64_t>(blocks, 1) <= 0x7FFFFFFFll, "ivf_search: too many row blocks for one query");
    }
    hipError_t e;
    if ((e = ivf->scores.ensure((size_t)per * ld * sizeof(double))) != hipSuccess ||
        (e = ivf->pids.ensure((size_t)per * np * sizeof(int64_t))) != hipSuccess ||
        (e = ivf->fval.ensure((size_t)per * np * sizeof(float))) != hipSuccess ||
        (e = ivf->probes.ensure((size_t)per * np * sizeof(int32_t))) != hipSuccess ||
        (e = ivf->qoff.ensure((size_t)per * (np + 1) * sizeof(int32_t))) != hipSuccess ||
        (e = pq ? pq_workspace(ivf, per, np) : scan_workspace(ivf, per, np)) != hipSuccess)
        return fail(MIRX_ENOMEM, std::string("ivf_search: workspace: ") + hipGetErrorString(e));
    for (int64_t q0 = 0; q0 < nq; q0 += per) {
        const SearchBatch b{q + q0 * ivf->dim, (int)std::min(per, nq - q0), np, ld, out_probes_or_null ? out_probes_or_null + q0 * np : nullptr};
        // the probes: the centroid index's own top-np (past mirx_index_search's k limit, its radix ranking: the same ranking)
        int rc = np <= MAX_K ? mirx_index_search(ivf->cent, b.qb, b.nb, np, nullptr, ivf->fval.as<float>(), ivf->pids.as<int64_t>(), st)
                             : mirx_index_rank_top(ivf->cent, b.qb, b.nb, np, nullptr, ivf->fval.as<float>(), nullptr,
                                                   ivf->pids.as<int64_t>(), st);
        if (rc) return rc;
        if ((rc = pq ? pq_scores(ivf, b, st) : scan_scores(ivf, b, st))) return rc;
        MIRX_HIP(launch_ivf_topk(ivf->scores.as<double>(), ld, ivf->probes.as<int32_t>(), ivf->qoff.as<int32_t>(), b.nb, np,
                                 ivf->offsets.as<int64_t>(), ivf->ids.as<int64_t>(),
                                 exclude_ids_or_null ? exclude_ids_or_null + q0 : nullptr, k, ivf->metric,
                                 out_f64_or_null ? out_f64_or_null + q0 * k : nullptr, out_ids + q0 * k,
                                 out_values_or_null ? out_values_or_null + q0 * k : nullptr, st));
        ++ivf->last_batches;
    }
    return MIRX_OK;
}

int mirx_ivf_last_stats(mirx_ivf *ivf, void *stream, mirx_ivf_stats *out) {
    MIRX_CHECK(ivf && out, "ivf_last_stats: null argument");
    MIRX_IVF_ENTER(ivf, "ivf_last_stats");
    unsigned long long v[3] = {0, 0, 0};
    MIRX_HIP(hipStreamSynchronize((hipStream_t)stream));
    MIRX_HIP(hipMemcpy(v, ivf->stats_dev, sizeof(v), hipMemcpyDeviceToHost));
    out->nq = ivf->last_nq;
    out->rows_scored = (int64_t)v[0];
    out->pairs = (int64_t)v[1];
    out->work_items = (int64_t)v[2];
    out->batches = ivf->last_batches;
    return MIRX_OK;
}

}  // extern "C"
