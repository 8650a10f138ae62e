// shard_merge.h — what the sharded index (shards.hip) needs of the merge across shards (shard_merge.hip): the ranks of one merge,
// the exchange between them, and the merge of the shards' device CSR answers.
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/coffeedb_gpu.h"
#include "common.h"

namespace cdb {

// exchange between the ranks of one merge (RCCL over distinct devices, device-to-device copies between ranks that share one)
struct Transport {
    virtual ~Transport() = default;
    // recv[q * bytes .. ) = rank q's `bytes` bytes of send, for every q
    virtual void all_gather(int rank, const void* send, void* recv, size_t bytes, hipStream_t s) = 0;
    // recv[off[q] * 8 .. ) = rank q's cnt[q] 8-byte elements of send (send holds cnt[rank] elements)
    virtual void all_gather_v(int rank, const void* send, void* recv, const uint64_t* cnt, const uint64_t* off, hipStream_t s) = 0;
    virtual const char* name() const = 0;
};

// The transport for the first G entries of `devices` as the ranks of ONE process (a host thread per rank calls the collectives):
// RCCL when the devices are distinct, RCCL is present and CDB_SHARD_TRANSPORT is not "copy"; otherwise — ranks that share a
// device, which RCCL refuses; a single rank — a board of published buffers and device-to-device copies.
std::shared_ptr<Transport> make_group_transport(int G, const std::vector<int>& devices);

// one rank of a merge: its place, its stream (its own, or borrowed from the shard whose answers it merges) and its work space
struct MergeRank {
    int rank = 0, world = 1, device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::shared_ptr<Transport> tr;
    DevBuf cnt, all_cnt, flat_ptr, g_row_ptr, offs, st_ids, st_cnt, out_ids, out_cnt, partials;
    mutable std::mutex err_mu;
    std::string err;
    ~MergeRank();
};

// collective over all ranks of mr.tr; local = this shard's device CSR; merged arrays live in mr
void merge_core(MergeRank& mr, const cdb_device_result& local, cdb_device_result& merged);

}  // namespace cdb
