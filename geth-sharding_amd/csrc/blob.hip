// Blob codec on gfx950 (sharding/utils/marshal.go:71-198), both directions; the per-chunk rules are
// blob_codec.h's, the same text tests/native/blob_codec_host.cpp runs on the CPU.
//
//   k_blob_serialize   utils.Serialize of a batch of blob lists.  The bodies of a batch are contiguous
//                      and each a multiple of 32 bytes, so the output is ONE array of 16-byte groups:
//                      lane g writes group g (half h = g & 1 of output chunk g >> 1) with one dwordx4
//                      store, consecutive lanes to consecutive addresses.  The plan (host, at prepare)
//                      gives a uint32 blob index per output chunk (4 bytes read per 32 written) and a
//                      16-byte entry per blob {offset, length, first chunk}, so a lane finds its blob in
//                      O(1).  A chunk's data starts at blob + 31 c, never aligned: the lane reads the
//                      up to five aligned dwords that hold its 16 source bytes and realigns them with a
//                      byte funnel shift (blob_codec.h serialize_group).  The terminal chunk's tail is
//                      masked to zero in registers; dwords wholly past the chunk's data are not loaded.
//                      No load leaves [blobs + begin, blobs + end): blob_codec.h load_dword.
//   k_blob_strip       the data half of utils.Deserialize: every indicator byte stripped, chunk c's 31
//                      bytes at 31 c of the body's data region (16 output bytes per lane, two aligned
//                      source dwords per output word).  The index half is notary.hip's k_blob_index.
//   k_blob_unpack      k_blob_index's records -> the arrays of the public interface.
//   k_proposer_mask    zeroes the outputs of the collations whose body exceeds 2^20 bytes.
#include <hip/hip_runtime.h>

#include "blob_codec.h"
#include "gsv_internal.h"

namespace gsv {

using namespace blobc;

// launch constants (tests/test_gpu_blob_codec.py places blobs across each of these boundaries)
constexpr int BS_THREADS = 256;                       // lanes per workgroup
constexpr int BS_GROUP_BYTES = GROUP;                 // 16: one lane's store
constexpr int BS_WAVE_BYTES = 64 * GROUP;             // 1,024: one wave's stores
constexpr int BS_BLOCK_BYTES = BS_THREADS * GROUP;    // 4,096: one workgroup's stores

__global__ __launch_bounds__(BS_THREADS) void k_blob_serialize(const uint8_t* __restrict__ blobs, uint64_t begin,
                                                              uint64_t end, const BlobEnt* __restrict__ ents,
                                                              const uint32_t* __restrict__ chunk_blob,
                                                              const uint8_t* __restrict__ skip_evm, uint64_t ngroups,
                                                              uint4* __restrict__ out) {
    const uint64_t g = (uint64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    if (g >= ngroups) return;
    const uint32_t cg = (uint32_t)(g >> 1), h = (uint32_t)(g & 1);
    const uint32_t k = chunk_blob[cg];
    const BlobEnt e = ents[k];
    const uint32_t c = cg - e.first;
    uint32_t f = 0;
    if (skip_evm && h == 0 && c + 1 == (uint32_t)num_chunks(e.len)) f = skip_evm[k];
    const Src s = make_src(blobs, begin, end);
    uint32_t w[4];
    serialize_group(s, e.off, e.len, f, c, h, w);
    out[g] = make_uint4(w[0], w[1], w[2], w[3]);
}

// grid (ceil(max groups / BS_THREADS), bodies): lane q of body b writes 16 bytes of its data region
__global__ __launch_bounds__(BS_THREADS) void k_blob_strip(const uint8_t* __restrict__ bodies, uint64_t begin,
                                                          uint64_t end, const uint64_t* __restrict__ body_off,
                                                          const uint32_t* __restrict__ body_len,
                                                          const uint64_t* __restrict__ data_off,
                                                          uint8_t* __restrict__ data) {
    const uint32_t b = blockIdx.y;
    const uint32_t q = blockIdx.x * BS_THREADS + threadIdx.x;
    const uint64_t o0 = data_off[b], o1 = data_off[b + 1];  // 16-byte aligned
    if ((uint64_t)q * GROUP >= o1 - o0) return;
    const uint32_t nch = body_len[b] / CHUNK;
    const Src s = make_src(bodies, begin, end);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = strip_word(s, body_off[b], nch, 4 * q + k);
    *(uint4*)(data + o0 + (uint64_t)q * GROUP) = make_uint4(w[0], w[1], w[2], w[3]);
}

// grid (ceil(max_blobs / 256), bodies)
__global__ __launch_bounds__(256) void k_blob_unpack(const BlobRec* __restrict__ recs, const uint32_t* __restrict__ cnt,
                                                    uint32_t max_blobs, uint32_t* __restrict__ start, uint32_t* __restrict__ len,
                                                    uint8_t* __restrict__ skip) {
    const uint32_t b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    if (t >= max_blobs) return;
    const size_t i = (size_t)b * max_blobs + t;
    BlobRec r{0, 0, 0, 0};
    if (t < cnt[b]) r = recs[i];
    start[i] = CHUNK_DATA * r.first_chunk;
    len[i] = r.len;
    skip[i] = (uint8_t)r.skip_evm;
}

__global__ __launch_bounds__(256) void k_proposer_mask(const uint8_t* __restrict__ over, uint32_t n, uint8_t* root32,
                                                      uint8_t* hash32, uint8_t* sig65, uint8_t* status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !over[i]) return;
    for (int k = 0; k < 32; k++) root32[(size_t)i * 32 + k] = 0;
    for (int k = 0; k < 32; k++) hash32[(size_t)i * 32 + k] = 0;
    for (int k = 0; k < 65; k++) sig65[(size_t)i * 65 + k] = 0;
    status[i] = GSV_ST_BODY_TOO_LARGE;
}

// d_out 16-byte aligned; nchunks output chunks in all (< 2^31)
hipError_t launch_blob_serialize(const uint8_t* d_blobs, uint64_t begin, uint64_t end, const void* d_ents,
                                 const uint32_t* d_chunk_blob, const uint8_t* d_skip_evm, uint64_t nchunks,
                                 uint8_t* d_out, hipStream_t st) {
    if (nchunks == 0) return hipSuccess;
    const uint64_t ngroups = 2 * nchunks;
    dim3 grid((uint32_t)((ngroups + BS_THREADS - 1) / BS_THREADS));
    hipLaunchKernelGGL(k_blob_serialize, grid, dim3(BS_THREADS), 0, st, d_blobs, begin, end, (const BlobEnt*)d_ents,
                       d_chunk_blob, d_skip_evm, ngroups, (uint4*)d_out);
    return hipGetLastError();
}

// max_region: the largest data region (bytes, a multiple of 16); d_data 16-byte aligned
hipError_t launch_blob_strip(const uint8_t* d_bodies, uint64_t begin, uint64_t end, const uint64_t* d_body_off,
                             const uint32_t* d_body_len, const uint64_t* d_data_off, uint32_t n, uint64_t max_region,
                             uint8_t* d_data, hipStream_t st) {
    if (n == 0 || max_region == 0) return hipSuccess;
    dim3 grid((uint32_t)((max_region / GROUP + BS_THREADS - 1) / BS_THREADS), n);
    hipLaunchKernelGGL(k_blob_strip, grid, dim3(BS_THREADS), 0, st, d_bodies, begin, end, d_body_off, d_body_len,
                       d_data_off, d_data);
    return hipGetLastError();
}

hipError_t launch_blob_unpack(const void* d_recs, const uint32_t* d_cnt, uint32_t n, uint32_t max_blobs,
                              uint32_t* d_start, uint32_t* d_len, uint8_t* d_skip, hipStream_t st) {
    if (n == 0) return hipSuccess;
    dim3 grid((max_blobs + 255) / 256, n);
    hipLaunchKernelGGL(k_blob_unpack, grid, dim3(256), 0, st, (const BlobRec*)d_recs, d_cnt, max_blobs, d_start,
                       d_len, d_skip);
    return hipGetLastError();
}

hipError_t launch_proposer_mask(const uint8_t* d_over, uint32_t n, uint8_t* d_root32, uint8_t* d_hash32,
                                uint8_t* d_sig65, uint8_t* d_status, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_proposer_mask, dim3((n + 255) / 256), dim3(256), 0, st, d_over, n, d_root32, d_hash32,
                       d_sig65, d_status);
    return hipGetLastError();
}

}  // namespace gsv
