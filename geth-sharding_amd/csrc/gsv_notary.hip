// Notary validation of the C ABI (gsv_ctx.h): blob decode + sender recovery beside the chunk roots of
// the same bodies, and the shard partition over ranks with its one RCCL all-gather.
#include <rccl/rccl.h>

#include "gsv_ctx.h"

using namespace gsv::api;

void gsv::api::comm_destroy(gsv_ctx* c) {
    if (c->comm) ncclCommDestroy(c->comm);
    c->comm = nullptr;
}

namespace {

// ---- notary: key = chain id, signer, max_txs, body offsets
std::vector<uint64_t> notary_key(const uint64_t* h_off, size_t n, const uint8_t* cid, size_t cidlen, int signer,
                                 uint32_t max_txs) {
    std::vector<uint64_t> k{(uint64_t)signer, max_txs};
    key_push_bytes(k, cid, cidlen);
    k.insert(k.end(), h_off, h_off + n + 1);
    return k;
}
int notary_shape(gsv_ctx* c, Shape& s, const uint64_t* start, const uint64_t* end, size_t n, const uint8_t* cid,
                 size_t cidlen, int signer_kind, uint32_t max_txs, Layout& L) {
    Shape::Notary& nt = s.notary;
    s.kind = SK_NOTARY;
    if (cidlen > 64) return GSV_E_INVALID_ARG;
    for (size_t i = 0; i < n; i++)
        if (end[i] < start[i] || end[i] - start[i] > MAX_BODY) return GSV_E_TOO_LARGE;
    // chain-id buffers: 64-byte big-endian value at 0 and the sighash suffix rlp(chainId) || 0x80 0x80
    // (<= 67 bytes) at 128, zero bytes around it (k_notary_tx reads it as aligned dwords)
    uint8_t host[256] = {0};
    if (cidlen) memcpy(host + 64 - cidlen, cid, cidlen);
    size_t z = 0;
    while (z < cidlen && cid[z] == 0) z++;
    size_t cn = cidlen - z, sl = 0;
    uint8_t* suf = host + 128;
    if (cn == 1 && cid[z] < 0x80) suf[sl++] = cid[z];
    else {
        suf[sl++] = (uint8_t)(0x80 + cn);
        if (cn) memcpy(suf + sl, cid + z, cn);
        sl += cn;
    }
    suf[sl++] = 0x80;
    suf[sl++] = 0x80;
    std::vector<uint64_t> offs(n);
    std::vector<uint32_t> lens(n);
    for (size_t i = 0; i < n; i++) {
        offs[i] = start[i];
        lens[i] = (uint32_t)(end[i] - start[i]);
    }
    nt.max_txs = max_txs;
    nt.signer_kind = signer_kind;
    nt.sfx_len = (uint32_t)sl;
    nt.o_cid = L.add(256);
    nt.o_noff = L.add(n * 8);
    nt.o_nlen = L.add(n * 4);
    nt.o_cnt = L.add(n * 4);
    nt.o_blobs = L.add((size_t)n * max_txs * gsv::blob_rec_bytes());
    s.stage(nt.o_cid, host, 256);
    s.stage(nt.o_noff, offs.data(), n);
    s.stage(nt.o_nlen, lens.data(), n);
    return chunk_prepare(c, s, s.chunk, L, start, end, n, MAX_BODY);
}
int notary_run(gsv_ctx* c, const Shape& s, size_t n, const uint8_t* d_bodies, uint8_t* d_root, uint32_t* d_ntx,
               uint8_t* d_bitmap, uint8_t* d_senders, uint8_t* d_status, hipStream_t st) {
    const Shape::Notary& nt = s.notary;
    size_t bm = (nt.max_txs + 7) / 8;
    uint32_t* d_cnt = d_ntx ? d_ntx : s.at<uint32_t>(nt.o_cnt);
    if (d_senders) HIPCHK(hipMemsetAsync(d_senders, 0, n * nt.max_txs * 20, st));
    if (d_status) HIPCHK(hipMemsetAsync(d_status, GSV_ST_BAD_RLP, n * nt.max_txs, st));
    // The chunk roots of the same bodies are independent of the transactions: with a side stream they
    // run beside the blob decode + recovery (fork / join by events, so a capture still works) and
    // fill the SIMDs the recovery kernel's tail and the trie top leave idle.
    // The chunk roots fork onto the shape's side stream when it has one (r03: +3.3 % against the serial
    // form, profiles/r03/ab_notary_fork.txt; r05: 11,491 vs 11,233 shards/s, profiles/r05/ab/notary_fork*.json)
    const bool fork = (size_t)s.cur < s.side.size();
    // The pipelined step's mark for the next step (GSV_HOOK_TAIL, shape_run) is the chunk root's, after
    // its bottom level.  r06 A/B at 13 / 25 / 100 shards, depth 2-4: no mark, or a mark after the blob
    // index, measured the same (profiles/r06/ab/notary_stagger_steps.txt).
    if (fork) {
        HIPCHK(hipEventRecord(s.efork[s.cur], st));
        HIPCHK(hipStreamWaitEvent(s.side[s.cur], s.efork[s.cur], 0));
        hipStream_t keep = c->cur_stream;
        c->cur_stream = s.side[s.cur];  // the chunk-root launch hooks time on the stream they run on
        int rc = chunk_run(c, s, s.chunk, d_bodies, d_root, s.side[s.cur]);
        c->cur_stream = keep;
        if (rc) return rc;
        HIPCHK(hipEventRecord(s.ejoin[s.cur], s.side[s.cur]));
    }
    hook_begin(c, GSV_K_NOTARY);
    HIPCHK(gsv::launch_blob_index(d_bodies, s.at<uint64_t>(nt.o_noff), s.at<uint32_t>(nt.o_nlen), (uint32_t)n,
                                  nt.max_txs, s.at<void>(nt.o_blobs), d_cnt, st));
    HIPCHK(gsv::launch_notary_tx(d_bodies, s.at<uint64_t>(nt.o_noff), s.at<void>(nt.o_blobs), d_cnt, (uint32_t)n,
                                 nt.max_txs, s.at<uint8_t>(nt.o_cid), s.at<uint8_t>(nt.o_cid) + 128, nt.sfx_len,
                                 nt.signer_kind, c->gtab, d_bitmap, (uint32_t)bm, d_senders, d_status, st));
    hook_end(c, GSV_K_NOTARY);
    if (fork) {
        HIPCHK(hipStreamWaitEvent(st, s.ejoin[s.cur], 0));
        return GSV_SUCCESS;
    }
    return chunk_run(c, s, s.chunk, d_bodies, d_root, st);  // chunk roots of the same bodies
}

// ---- shard partition: the notary shape of this rank's block + its record block and the gathered
// blocks; key = notary key of the block + (n_total, nranks, rank)
std::vector<uint64_t> partition_key(const uint64_t* h_off, size_t n, size_t n_total, int N, int r, const uint8_t* cid,
                                    size_t cidlen, int signer, uint32_t max_txs) {
    std::vector<uint64_t> k = notary_key(h_off, n, cid, cidlen, signer, max_txs);
    k.push_back(n_total);
    k.push_back((uint64_t)N);
    k.push_back((uint64_t)r);
    return k;
}
int partition_shape(gsv_ctx* c, Shape& s, const uint64_t* h_off, size_t n_total, int N, int r, const uint8_t* cid,
                    size_t cidlen, int signer_kind, uint32_t max_txs, Layout& L) {
    PartDims d = part_dims(n_total, N, r, max_txs);
    if (d.n) {  // the rank's own block: s.notary and s.chunk, as in a notary shape
        int rc = notary_shape(c, s, h_off, h_off + 1, d.n, cid, cidlen, signer_kind, max_txs, L);
        if (rc) return rc;
    }
    s.kind = SK_PARTITION;
    s.notary.max_txs = max_txs;
    s.part.n = d.n;
    s.part.total = n_total;
    s.part.ranks = N;
    s.part.rank = r;
    s.part.o_lroot = L.add(d.n * 32);
    s.part.o_lntx = L.add(d.n * 4);
    s.part.o_lbm = L.add(d.n * d.bm);
    s.part.o_block = L.add(d.B);
    s.part.o_all = L.add((size_t)N * d.B);
    return GSV_SUCCESS;
}
// validate the rank's block and pack its records into `blk`
int partition_pack(gsv_ctx* c, const Shape& s, const PartDims& d, const uint8_t* d_bodies, uint8_t* d_senders,
                   uint8_t* d_status, uint8_t* blk, hipStream_t st) {
    uint8_t* lroot = s.at<uint8_t>(s.part.o_lroot);
    uint32_t* lntx = s.at<uint32_t>(s.part.o_lntx);
    uint8_t* lbm = s.at<uint8_t>(s.part.o_lbm);
    if (d.n) {
        int rc = notary_run(c, s, d.n, d_bodies, lroot, lntx, lbm, d_senders, d_status, st);
        if (rc) return rc;
    }
    return hip_err(gsv::launch_partition_pack(lroot, lntx, lbm, (uint32_t)d.n, (uint32_t)d.per, (uint32_t)d.R,
                                              (uint32_t)d.bm, 0, blk, st));
}
// the path's one collective: every rank's block to every rank (one ncclAllGather over xGMI)
int partition_gather(gsv_ctx* c, const uint8_t* blk, uint8_t* all, const PartDims& d, hipStream_t st) {
    if (c->comm) {  // any communicator, one rank included: the same chain on every rank count
        std::lock_guard<std::mutex> g(c->cmu);  // callers hold mu (error path) or smu (success path)
        // calls kept in flight on several streams (pipeline depth) overlap their validation, not their
        // collectives: each all-gather follows the previous one on the communicator (every rank issues
        // them in the same order).  Inside a graph capture the caller's graph orders them.
        const bool cap = capturing(st);
        if (!cap) {
            if (!c->coll_ev && hipEventCreateWithFlags(&c->coll_ev, hipEventDisableTiming) != hipSuccess)
                return GSV_E_HIP;
            if (c->coll_rec && hipStreamWaitEvent(st, c->coll_ev, 0) != hipSuccess) return GSV_E_HIP;
        }
        if (ncclAllGather(blk, all, d.B, ncclUint8, c->comm, st) != ncclSuccess) return GSV_E_RCCL;
        if (!cap) {
            if (hipEventRecord(c->coll_ev, st) != hipSuccess) return GSV_E_HIP;
            c->coll_rec = true;
        }
        return GSV_SUCCESS;
    }
    if (c->nranks > 1) return GSV_E_INVALID_ARG;
    return hip_err(hipMemcpyAsync(all, blk, d.B, hipMemcpyDeviceToDevice, st));
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ notary validation (configs[3])
int gsv_notary_synth_dev(gsv_ctx* c, uint64_t seed, uint32_t shard0, size_t n_shards, uint32_t txs_per_shard,
                         uint8_t* d_bodies, uint8_t* d_exp_status, uint8_t* d_exp_sender, void* stream) {
    if (!c || (n_shards && !d_bodies) || (uint64_t)n_shards * txs_per_shard > 0xFFFFFFFFull) return GSV_E_INVALID_ARG;
    HIPCHK(hipSetDevice(c->device));
    return hip_err(gsv::launch_notary_synth(seed, shard0, (uint32_t)n_shards, txs_per_shard, c->gtab, d_bodies,
                                            d_exp_status, d_exp_sender, stream_of(c, stream)));
}

static int notary_args(const uint8_t* chain_id, size_t chain_id_len, int signer_kind, size_t n_shards,
                       uint32_t max_txs) {
    if ((chain_id_len && !chain_id) || chain_id_len > 64 || signer_kind < GSV_SIGNER_EIP155 ||
        signer_kind > GSV_SIGNER_FRONTIER)
        return GSV_E_INVALID_ARG;
    // every blob takes at least one 32-byte chunk, so a body of at most 2^20 bytes holds at most
    // GSV_MAX_TXS_PER_SHARD = 32,768 of them (also keeps the partition's record offsets in 32 bits)
    if (n_shards > 65535 || max_txs == 0 || max_txs > GSV_MAX_TXS_PER_SHARD) return GSV_E_INVALID_ARG;
    return GSV_SUCCESS;
}

int gsv_notary_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n_shards, const uint8_t* chain_id,
                       size_t chain_id_len, int signer_kind, uint32_t max_txs) {
    if (!c || (n_shards && !h_off)) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_shards, max_txs);
    if (rc || n_shards == 0) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    rc = shape_get(c, SK_NOTARY, notary_key(h_off, n_shards, chain_id, chain_id_len, signer_kind, max_txs),
                   [&](Shape& ns, Layout& L) {
                       return notary_shape(c, ns, h_off, h_off + 1, n_shards, chain_id, chain_id_len, signer_kind,
                                           max_txs, L);
                   },
                   &s);
    if (rc) return rc;
    return shape_side_init(c, *s);
}

int gsv_notary_validate_shards_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n_shards,
                                   const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                                   uint8_t* d_root32, uint32_t* d_ntx, uint8_t* d_bitmap, uint8_t* d_senders,
                                   uint8_t* d_status, void* stream) {
    if (!c || (n_shards && (!d_bodies || !h_off || !d_root32 || !d_bitmap))) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_shards, max_txs);
    if (rc || n_shards == 0) return rc;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_NOTARY, notary_key(h_off, n_shards, chain_id, chain_id_len, signer_kind, max_txs));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] {
        return notary_run(c, *s, n_shards, d_bodies, d_root32, d_ntx, d_bitmap, d_senders, d_status, st);
    });
}

int gsv_notary_validate_shards(gsv_ctx* c, const uint8_t* bodies, const uint64_t* off, size_t n_shards,
                               const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                               uint8_t* root32_out, uint32_t* ntx_out, uint8_t* valid_bitmap_out,
                               uint8_t* senders_out, uint8_t* status_out) {
    if (!c || (n_shards && (!bodies || !off || !root32_out || !ntx_out || !valid_bitmap_out))) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_shards, max_txs);
    if (rc || n_shards == 0) return rc;
    GSVCHK(table_check(bodies, off, n_shards, kBodies));
    std::vector<uint64_t> st, en;
    uint64_t pos = stage_offsets(off, n_shards, st, en);
    Layout staged;
    const NotaryStage p(staged, pos, n_shards, max_txs, senders_out != nullptr, status_out != nullptr);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    GSVCHK(shape_temp(c, staged,
                      [&](Shape& ns, Layout& L) {
                          return notary_shape(c, ns, st.data(), en.data(), n_shards, chain_id, chain_id_len,
                                              signer_kind, max_txs, L);
                      },
                      s));
    GSVCHK(shape_side_borrow(c, s));
    uint8_t* d_b = sg(p.bodies);
    GSVCHK(stage_bodies(c, d_b, bodies, off, n_shards, st, en));
    GSVCHK(shape_run(c, s, c->stream, [&] {
        // sg(p.senders), sg(p.status): nullptr when not asked for
        return notary_run(c, s, n_shards, d_b, sg(p.root), sg(p.ntx), sg(p.bitmap), sg(p.senders), sg(p.status),
                          c->stream);
    }));
    GSVCHK(sg.out(root32_out, p.root));
    GSVCHK(sg.out(ntx_out, p.ntx));
    GSVCHK(sg.out(valid_bitmap_out, p.bitmap));
    GSVCHK(sg.out(senders_out, p.senders));
    GSVCHK(sg.out(status_out, p.status));
    GSVCHK(sg.finish());
    for (size_t i = 0; i < n_shards; i++)
        if (ntx_out[i] > max_txs) return GSV_E_TOO_LARGE;
    return GSV_SUCCESS;
}

// ------------------------------------------------------------------ shard partition + RCCL all-gather
// Record per shard (the layout of gsv/shards.py): root 32 | ntx 4 | bitmap ceil(max_txs/8), padded to
// 8 bytes.  Each rank packs its block's records with three strided copies, one ncclAllGather moves
// every rank's block (ceil(S/N) records, the tail of a short block unused), and three strided copies
// per rank unpack the gathered records into shard order.
int gsv_comm_unique_id(uint8_t id[GSV_COMM_ID_BYTES]) {
    if (!id) return GSV_E_INVALID_ARG;
    static_assert(sizeof(ncclUniqueId) == GSV_COMM_ID_BYTES, "RCCL unique id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return GSV_E_RCCL;
    memcpy(id, &u, sizeof(u));
    return GSV_SUCCESS;
}

int gsv_comm_init(gsv_ctx* c, const uint8_t id[GSV_COMM_ID_BYTES], int nranks, int rank) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(hipSetDevice(c->device));
    if (c->comm) {
        ncclCommDestroy(c->comm);
        c->comm = nullptr;
    }
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    if (ncclCommInitRank(&c->comm, nranks, u, rank) != ncclSuccess) {
        c->comm = nullptr;
        return GSV_E_RCCL;
    }
    c->nranks = nranks;
    c->rank = rank;
    return GSV_SUCCESS;
}

int gsv_comm_info(gsv_ctx* c, int* nranks, int* rank) {
    if (!c) return GSV_E_INVALID_ARG;
    if (nranks) *nranks = c->nranks;
    if (rank) *rank = c->rank;
    return GSV_SUCCESS;
}

int gsv_shard_range(size_t n_shards, int nranks, int rank, size_t* first, size_t* count) {
    if (nranks < 1 || rank < 0 || rank >= nranks || !first || !count) return GSV_E_INVALID_ARG;
    size_t a = n_shards * (size_t)rank / (size_t)nranks, b = n_shards * (size_t)(rank + 1) / (size_t)nranks;
    *first = a;
    *count = b - a;
    return GSV_SUCCESS;
}

size_t gsv_partition_block_bytes(size_t n_total, int nranks, uint32_t max_txs) {
    if (nranks < 1) return 0;
    return part_dims(n_total, nranks, 0, max_txs).B;
}

int gsv_notary_partition_prepare(gsv_ctx* c, const uint64_t* h_off, size_t n_total, int nranks, int rank,
                                 const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs) {
    if (!c || !h_off || nranks < 1 || rank < 0 || rank >= nranks) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_total, max_txs);
    if (rc) return rc;
    if (n_total > 0xFFFFFFFFull / 4096) return GSV_E_TOO_LARGE;
    PartDims d = part_dims(n_total, nranks, rank, max_txs);
    std::lock_guard<std::mutex> g(c->smu);
    HIPCHK(hipSetDevice(c->device));
    Shape* s;
    rc = shape_get(c, SK_PARTITION,
                   partition_key(h_off, d.n, n_total, nranks, rank, chain_id, chain_id_len, signer_kind, max_txs),
                   [&](Shape& ns, Layout& L) {
                       return partition_shape(c, ns, h_off, n_total, nranks, rank, chain_id, chain_id_len,
                                              signer_kind, max_txs, L);
                   },
                   &s);
    if (rc) return rc;
    return d.n ? shape_side_init(c, *s) : GSV_SUCCESS;
}

int gsv_notary_partition_pack_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n_total,
                                  int nranks, int rank, const uint8_t* chain_id, size_t chain_id_len, int signer_kind,
                                  uint32_t max_txs, uint8_t* d_block, uint8_t* d_senders, uint8_t* d_status,
                                  void* stream) {
    if (!c || !h_off || !d_block || nranks < 1 || rank < 0 || rank >= nranks) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_total, max_txs);
    if (rc) return rc;
    PartDims d = part_dims(n_total, nranks, rank, max_txs);
    if (d.n && !d_bodies) return GSV_E_INVALID_ARG;
    std::lock_guard<std::mutex> g(c->smu);
    Shape* s = shape_find(c, SK_PARTITION,
                          partition_key(h_off, d.n, n_total, nranks, rank, chain_id, chain_id_len, signer_kind, max_txs));
    if (!s) return GSV_E_NOT_PREPARED;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return shape_run(c, *s, st, [&] { return partition_pack(c, *s, d, d_bodies, d_senders, d_status, d_block, st); });
}

int gsv_notary_partition_unpack_dev(gsv_ctx* c, const uint8_t* d_blocks, size_t n_total, int nranks, uint32_t max_txs,
                                    uint8_t* d_root32_all, uint32_t* d_ntx_all, uint8_t* d_bitmap_all,
                                    int32_t* d_rank_status, void* stream) {
    if (!c || !d_blocks || nranks < 1 || max_txs == 0 || (n_total && (!d_root32_all || !d_ntx_all || !d_bitmap_all)))
        return GSV_E_INVALID_ARG;
    if (n_total > 0xFFFFFFFFull / 4096) return GSV_E_TOO_LARGE;
    PartDims d = part_dims(n_total, nranks, 0, max_txs);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    return hip_err(gsv::launch_partition_unpack(d_blocks, (uint32_t)nranks, (uint32_t)n_total, (uint32_t)d.R,
                                                (uint32_t)d.bm, d.B, d_root32_all, d_ntx_all, d_bitmap_all,
                                                d_rank_status, st));
}

int gsv_notary_validate_partition_dev(gsv_ctx* c, const uint8_t* d_bodies, const uint64_t* h_off, size_t n_total,
                                      const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                                      uint8_t* d_root32_all, uint32_t* d_ntx_all, uint8_t* d_bitmap_all,
                                      uint8_t* d_senders, uint8_t* d_status, int32_t* d_rank_status, void* stream) {
    // arguments every rank passes alike: an error here is the same error on every rank, and no rank
    // enters the collective
    if (!c || (n_total && (!d_root32_all || !d_ntx_all || !d_bitmap_all))) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_total, max_txs);
    if (rc || n_total == 0) return rc;
    if (n_total > 0xFFFFFFFFull / 4096) return GSV_E_TOO_LARGE;
    const int N = c->nranks, r = c->rank;
    PartDims d = part_dims(n_total, N, r, max_txs);
    hipStream_t st = stream_of(c, stream);
    // rank-local failures still reach the all-gather with the rank's status in its block header
    int lrc = (!h_off || (d.n && !d_bodies)) ? GSV_E_INVALID_ARG : GSV_SUCCESS;
    bool joined = false;  // this rank has entered the all-gather
    if (!lrc) {
        std::lock_guard<std::mutex> g(c->smu);
        Shape* s = shape_find(c, SK_PARTITION, partition_key(h_off, d.n, n_total, N, r, chain_id, chain_id_len,
                                                             signer_kind, max_txs));
        if (!s) lrc = GSV_E_NOT_PREPARED;
        else if (hipSetDevice(c->device) != hipSuccess) lrc = GSV_E_HIP;
        else {
            lrc = shape_run(c, *s, st, [&] {
                uint8_t* blk = s->at<uint8_t>(s->part.o_block);
                uint8_t* all = s->at<uint8_t>(s->part.o_all);
                int e = partition_pack(c, *s, d, d_bodies, d_senders, d_status, blk, st);
                if (e) return e;
                joined = true;
                e = partition_gather(c, blk, all, d, st);
                if (e) return e;
                return hip_err(gsv::launch_partition_unpack(all, (uint32_t)N, (uint32_t)n_total, (uint32_t)d.R,
                                                            (uint32_t)d.bm, d.B, d_root32_all, d_ntx_all,
                                                            d_bitmap_all, d_rank_status, st));
            });
            if (!lrc || joined) return lrc;  // done, or failed at/after the collective: nothing more to join
        }
    }
    // error path: join the collective from the staging arena with this rank's status and no records
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return lrc;
    Layout L;
    const B8 b_blk = L.buf(d.B), b_all = L.buf((size_t)N * d.B);
    if (arena_reserve(c, L.n)) return lrc;
    uint8_t *blk = b_blk(c->arena), *all = b_all(c->arena);
    if (gsv::launch_partition_pack(nullptr, nullptr, nullptr, 0, (uint32_t)d.per, (uint32_t)d.R, (uint32_t)d.bm, lrc,
                                   blk, st) != hipSuccess)
        return lrc;
    if (partition_gather(c, blk, all, d, st)) return lrc;
    gsv::launch_partition_unpack(all, (uint32_t)N, (uint32_t)n_total, (uint32_t)d.R, (uint32_t)d.bm, d.B,
                                 d_root32_all, d_ntx_all, d_bitmap_all, d_rank_status, st);
    hipStreamSynchronize(st);  // the arena is reused by the next host-path call
    return lrc;
}

int gsv_notary_validate_partition(gsv_ctx* c, const uint8_t* bodies, const uint64_t* off, size_t n_total,
                                  const uint8_t* chain_id, size_t chain_id_len, int signer_kind, uint32_t max_txs,
                                  uint8_t* root32_all, uint32_t* ntx_all, uint8_t* bitmap_all,
                                  uint8_t* senders_out, uint8_t* status_out) {
    // arguments every rank passes alike (see the _dev form)
    if (!c || !off || (n_total && (!root32_all || !ntx_all || !bitmap_all))) return GSV_E_INVALID_ARG;
    int rc = notary_args(chain_id, chain_id_len, signer_kind, n_total, max_txs);
    if (rc || n_total == 0) return rc;
    if (n_total > 0xFFFFFFFFull / 4096) return GSV_E_TOO_LARGE;
    const int N = c->nranks, r = c->rank;
    PartDims d = part_dims(n_total, N, r, max_txs);
    const size_t n = d.n;
    hipStream_t sm = c->stream;
    int lrc = (n && !bodies) ? GSV_E_INVALID_ARG : GSV_SUCCESS;
    if (!lrc) lrc = table_check(bodies, off, n, kBodies);
    std::vector<uint64_t> st, en;
    uint64_t pos = n && !lrc ? stage_offsets(off, n, st, en) : 0;
    // gathered outputs + statuses first in the arena (PartitionStage), so a rank whose block failed
    // reserves those alone, finds them at the same place and still joins the collective
    Layout staged;
    const PartitionStage p(staged, d, n_total, N, pos, max_txs, senders_out != nullptr, status_out != nullptr);
    Staged sg(c, staged, Staged::kWithShape);
    if (sg.rc) return sg.rc;
    std::lock_guard<std::mutex> g2(c->smu);
    Shape s;
    if (!lrc) {
        lrc = shape_temp(c, staged,
                         [&](Shape& ns, Layout& L) {
                             if (!n) return GSV_SUCCESS;
                             return notary_shape(c, ns, st.data(), en.data(), n, chain_id, chain_id_len, signer_kind,
                                                 max_txs, L);
                         },
                         s);
        if (!lrc && n) lrc = shape_side_borrow(c, s);
    }
    if (lrc && arena_reserve(c, p.gathered)) return lrc;  // cannot even join the collective
    uint8_t *d_blk = sg(p.blk), *d_all = sg(p.all);
    uint8_t *d_snd = sg(p.own.senders), *d_st = sg(p.own.status);  // used on success only
    if (!lrc) {
        uint8_t *d_b = sg(p.own.bodies), *d_r = sg(p.own.root), *d_bm = sg(p.own.bitmap);
        uint32_t* d_n = sg(p.own.ntx);
        if (n) lrc = stage_bodies(c, d_b, bodies, off, n, st, en);
        if (!lrc && n)
            lrc = shape_run(c, s, sm, [&] { return notary_run(c, s, n, d_b, d_r, d_n, d_bm, d_snd, d_st, sm); });
        if (!lrc)
            lrc = hip_err(gsv::launch_partition_pack(d_r, d_n, d_bm, (uint32_t)n, (uint32_t)d.per, (uint32_t)d.R,
                                                     (uint32_t)d.bm, 0, d_blk, sm));
    }
    if (lrc && gsv::launch_partition_pack(nullptr, nullptr, nullptr, 0, (uint32_t)d.per, (uint32_t)d.R,
                                          (uint32_t)d.bm, lrc, d_blk, sm) != hipSuccess)
        return lrc;
    int grc = partition_gather(c, d_blk, d_all, d, sm);
    if (grc) return grc;
    HIPCHK(gsv::launch_partition_unpack(d_all, (uint32_t)N, (uint32_t)n_total, (uint32_t)d.R, (uint32_t)d.bm, d.B,
                                        sg(p.oroot), sg(p.ontx), sg(p.obm), sg(p.rst), sm));
    std::vector<int32_t> rst(N);
    GSVCHK(sg.out(root32_all, p.oroot));
    GSVCHK(sg.out(ntx_all, p.ontx));
    GSVCHK(sg.out(bitmap_all, p.obm));
    GSVCHK(sg.out(rst.data(), p.rst));
    if (!lrc && n) {  // the own block's buffers were reserved and written
        GSVCHK(sg.out(senders_out, p.own.senders));
        GSVCHK(sg.out(status_out, p.own.status));
    }
    GSVCHK(sg.finish());
    // every rank returns the same verdict: the status of the lowest failing rank
    for (int q = 0; q < N; q++)
        if (rst[q]) return rst[q];
    for (size_t i = 0; i < n_total; i++)
        if (ntx_all[i] > max_txs) return GSV_E_TOO_LARGE;
    return GSV_SUCCESS;
}

}  // extern "C"
