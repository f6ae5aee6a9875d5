// comm.h -- the transports of a context (comm.cpp, k_comm.hip, xch_dev.h): RCCL, the in-process loopback
// hub and the xGMI mailboxes, and what comm.cpp offers the rest of the library.  A part of internal.h,
// which includes it after its typedefs and error macros; sources include internal.h.
#pragma once
#include <rccl/rccl.h>

#include <condition_variable>
#include <mutex>
#include <vector>

struct eig_mat_s;

namespace eigmi {

#define EIG_NCCL(call)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (call);                                                                  \
    if (r_ != ncclSuccess)                                                                     \
      throw ::eigmi::Error(EIG_ERR_RCCL, std::string(#call) + ": " + ncclGetErrorString(r_));  \
  } while (0)

// In-process loopback transport: P virtual ranks (one host thread + context each, usually on the
// same device) exchange through this hub instead of RCCL.  Test-only path for the distributed
// code on a single GPU; every operation is synchronous.
struct LoopHub {
  explicit LoopHub(int n) : P(n), xptr(n), win_begin(n), red(n), gather(4 * (size_t)n), mbox(n), flag(n) {}
  int P;
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  unsigned long gen = 0;
  std::vector<double *> xptr;      // per rank: vector being exchanged
  std::vector<i64> win_begin;      // per rank: window begin (scalar)
  std::vector<std::vector<double>> red;
  std::vector<i64> gather;
  std::vector<u64 *> mbox;                 // per rank: its mailbox (eig_comm_loopback_mailbox)
  std::vector<int> flag;                   // per rank: a flag agreed through the hub
  void barrier()
  {
    std::unique_lock<std::mutex> lk(m);
    const unsigned long g = gen;
    if (++arrived == P)
    {
      arrived = 0;
      ++gen;
      cv.notify_all();
    }
    else
      cv.wait(lk, [&] { return gen != g; });
  }
};

// Host-side ownership of a region that peer processes map over HIP IPC (both mailboxes are one): an uncached,
// exported allocation and a small private state block, both zeroed, plus the peers' regions opened here.
struct IpcRegion {
  void *base = nullptr;          // hipExtMallocWithFlags allocation (exported)
  size_t bytes = 0;              // its size
  void *state = nullptr;         // hipMalloc
  std::vector<void *> opened;    // IPC-opened peer mappings (closed on release)
  void alloc(size_t region_bytes, size_t state_bytes);
  void export_handle(unsigned char handle[HIP_IPC_HANDLE_SIZE]) const;
  void *open_peer(const unsigned char handle[HIP_IPC_HANDLE_SIZE]);
  void release();  // closes the mappings, then frees the allocation, then the state
};

// xGMI mailbox allreduce (k_comm.hip): each rank's uncached mailbox, IPC-mapped by every peer.
constexpr int kMaxMailboxRanks = 16;
constexpr int kMailboxVals = 63;  // values per call (slot = 1 sequence word + 63 values = 512 B)
constexpr int kXchWords = 4;       // step region slot (xch_dev.h): sequence number + 3 sums
struct Mailbox {
  u64 *local = nullptr;                  // my mailbox: [2][P][1 + kMailboxVals], then the step region
  u64 *peer[kMaxMailboxRanks] = {};      // peer[r] = rank r's mailbox mapped here (peer[me] = local)
  u64 *ctr = nullptr;                    // device: sequence number of the last completed call
  u64 *fctr = nullptr;                   // device: sequence number of the last fused-step exchange
  int *err = nullptr;                    // device: set when a call timed out
  long long foff = 0;                    // word offset of the step region [2][P][kXchWords] (xch_dev.h)
  int P = 1, me = 0;
};
// Host-side ownership of the mailbox resources of a context.
struct MailboxHost {
  Mailbox dev;
  IpcRegion mem;                 // the mailbox; state = ctr + fctr + err (256 B)
  bool ready = false;            // peers opened and validated: allreduce_sum uses it
  bool on = true;                // eig_comm_select_allreduce: false = ncclAllReduce although ready
  bool step = false;             // EIG_AR_MAILBOX_STEP: the fused step exchanges its sums in-kernel
};
constexpr unsigned long long kMailboxTimeout = 1000000000ull;  // 10 s of s_memrealtime (100 MHz)
void launch_mailbox_allreduce(double *buf, int count, const Mailbox &mb, unsigned long long timeout, hipStream_t s);

// xGMI halo mailbox (k_comm.hip) of mailbox-only ranks (eig_comm_ipc_open, no RCCL): every rank's
// uncached staging area, IPC-mapped by every peer.  Layout: [2][P] sequence lines (one 128-B line
// per word), then [2][P][cap] doubles; parity = sequence & 1, slot = the sending rank.
constexpr int kHaloFlagStride = 16;  // u64 words per sequence line
struct HaloBox {
  u64 *flags = nullptr;                         // mine: [2][P] lines
  u64 *peer_flags[kMaxMailboxRanks] = {};       // rank r's lines mapped here (peer_flags[me] = flags)
  double *stage = nullptr;                      // mine: [2][P][cap]
  double *peer_stage[kMaxMailboxRanks] = {};
  u64 *seq = nullptr;                           // device: [P] exchanges completed with each peer
  unsigned *ticket = nullptr;                   // device: push / pull last-workgroup tickets (128 B apart)
  int *err = nullptr;                           // the mailbox's error word (Mailbox::err)
  long long cap = 0;                            // doubles per slot
  int P = 1, me = 0;
};
struct HaloBoxHost {
  HaloBox dev;
  IpcRegion mem;                 // the staging area; state = seq + tickets (512 B)
};
// One side of an exchange: n ranges (peer, window offset, count) in scalar units.
struct HaloXfer {
  int n = 0;
  int peer[kMaxMailboxRanks] = {};
  long long off[kMaxMailboxRanks] = {};
  long long cnt[kMaxMailboxRanks] = {};
};
void launch_halo_mailbox(const HaloBox &hb, const HaloXfer &snd, const HaloXfer &rcv, const HaloXfer &sync, double *x,
                         double *x2, int width, hipStream_t s);

// ---- comm.cpp --------------------------------------------------------------------------------
// Ghost entries of window vector x (and x2 when given) from their owners.
// width: doubles per row of x (2 for the fused step's interleaved pair vectors).
void halo_exchange(const eig_mat_s &A, double *x, hipStream_t s, double *x2 = nullptr, int width = 1);
void allreduce_sum(eig_ctx_t ctx, double *buf, i64 count, hipStream_t s);
// Whether allreduce_sum_red can run on ctx->red_stream concurrently with the compute and halo
// streams (RCCL with the split communicator, or the mailbox); false for one rank / loopback.
bool allreduce_overlaps(eig_ctx_t ctx);
// allreduce_sum on the split communicator (or the mailbox), for ctx->red_stream.
void allreduce_sum_red(eig_ctx_t ctx, double *buf, i64 count, hipStream_t s);
// Allgather of every rank's 4 values `mine` (row_begin, nb_local, cmin, cmax) over the context's transport.
std::vector<i64> allgather_rows(eig_ctx_t ctx, const std::vector<i64> &mine);
// The halo mailbox's staging holds the largest receive range of any rank's plan (`all`: allgather_rows'
// result, bc: scalars per block column), 8 columns wide; grown, collectively, when this matrix needs more.
void halo_staging_ensure(eig_ctx_t ctx, const std::vector<i64> &all, int bc);
// Releases the context's transports: the mailboxes, then the split communicator, then the communicator.
void comm_destroy(eig_ctx_t ctx);

}  // namespace eigmi
