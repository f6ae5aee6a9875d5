// comm.cpp -- the communication layer of libeigmi (comm.h): the RCCL communicator and its split, the
// in-process loopback hub, the xGMI mailbox allreduce (prepare, open, validate, restart), the halo mailbox
// staging and the three-way halo exchange, the allgather of the distributed create, and every
// eig_comm_* / eig_loopback_* entry point.  The mailbox kernels live in k_comm.hip and xch_dev.h.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "internal.h"

using namespace eigmi;

namespace eigmi {

void IpcRegion::alloc(size_t region_bytes, size_t state_bytes)
{
  // uncached: a peer's stores over xGMI land in HBM and my polling loads must see them while
  // the kernel runs; fine-grained is the fallback where uncached memory cannot be exported
  void *p = nullptr;
  if (hipExtMallocWithFlags(&p, region_bytes, hipDeviceMallocUncached) != hipSuccess)
  {
    (void)hipGetLastError();
    EIG_HIP(hipExtMallocWithFlags(&p, region_bytes, hipDeviceMallocFinegrained));
  }
  base = p;
  bytes = region_bytes;
  EIG_HIP(hipMemset(base, 0, bytes));
  EIG_HIP(hipMalloc(&state, state_bytes));
  EIG_HIP(hipMemset(state, 0, state_bytes));
}

void IpcRegion::export_handle(unsigned char handle[HIP_IPC_HANDLE_SIZE]) const
{
  hipIpcMemHandle_t h;
  EIG_HIP(hipIpcGetMemHandle(&h, base));
  std::memcpy(handle, &h, HIP_IPC_HANDLE_SIZE);
}

void *IpcRegion::open_peer(const unsigned char handle[HIP_IPC_HANDLE_SIZE])
{
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, HIP_IPC_HANDLE_SIZE);
  void *p = nullptr;
  EIG_HIP(hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess));
  opened.push_back(p);
  return p;
}

void IpcRegion::release()
{
  for (void *p : opened) (void)hipIpcCloseMemHandle(p);
  if (base) (void)hipFree(base);
  if (state) (void)hipFree(state);
  *this = IpcRegion();
}

namespace {

// Runs f; false when it threw a library error (the callers then agree on the outcome with their peers).
template <class F>
bool succeeds(F &&f)
{
  try
  {
    f();
    return true;
  }
  catch (const Error &)
  {
    return false;
  }
}

// The mailbox allreduce of `count` doubles, kMailboxVals per launch.
void mailbox_sum(eig_ctx_t ctx, double *buf, i64 count, hipStream_t s)
{
  for (i64 off = 0; off < count; off += kMailboxVals)
    launch_mailbox_allreduce(buf + off, (int)std::min<i64>(kMailboxVals, count - off), ctx->mbox->dev, kMailboxTimeout,
                             s);
}

// Zero one double, sum it over the ranks on ctx->stream and wait: no rank returns before every rank is here.
void stream_barrier(eig_ctx_t ctx)
{
  double *d = ctx->scratch + 4000;
  EIG_HIP(hipMemsetAsync(d, 0, sizeof(double), ctx->stream));
  allreduce_sum(ctx, d, 1, ctx->stream);
  EIG_HIP(hipStreamSynchronize(ctx->stream));
}

// xGMI mailbox (k_comm.hip).  prepare: allocate my uncached mailbox + state and export it;
// open: map every peer's mailbox; validate: one allreduce of rank+1 must give P(P+1)/2 exactly.
void halobox_free(eig_ctx_t ctx)
{
  HaloBoxHost *h = ctx->hbox;
  if (!h) return;
  h->mem.release();
  delete h;
  ctx->hbox = nullptr;
}

void mailbox_free(eig_ctx_t ctx)
{
  halobox_free(ctx);  // its error word is the mailbox's
  MailboxHost *m = ctx->mbox;
  if (!m) return;
  m->mem.release();
  delete m;
  ctx->mbox = nullptr;
}

void mailbox_prepare(eig_ctx_t ctx, int nranks, int rank, unsigned char handle[HIP_IPC_HANDLE_SIZE])
{
  EIG_CHECK(nranks >= 1 && nranks <= kMaxMailboxRanks && rank >= 0 && rank < nranks, EIG_ERR_ARG,
            "mailbox: rank count outside 1..16");
  mailbox_free(ctx);
  auto *m = new MailboxHost();
  ctx->mbox = m;
  // k_comm.hip region [2][P][1 + kMailboxVals], then the fused step's region [2][P][kXchWords]
  const size_t foff = (size_t)2 * nranks * (1 + kMailboxVals);
  m->mem.alloc((foff + (size_t)2 * nranks * kXchWords) * sizeof(u64), 256);
  char *state = static_cast<char *>(m->mem.state);
  m->dev.local = static_cast<u64 *>(m->mem.base);
  m->dev.ctr = reinterpret_cast<u64 *>(state);
  m->dev.fctr = reinterpret_cast<u64 *>(state + 64);
  m->dev.err = reinterpret_cast<int *>(state + 128);
  m->dev.foff = (long long)foff;
  m->dev.P = nranks;
  m->dev.me = rank;
  m->mem.export_handle(handle);
}

void mailbox_open(eig_ctx_t ctx, const unsigned char *handles)
{
  MailboxHost *m = ctx->mbox;
  EIG_CHECK(m && m->mem.base, EIG_ERR_ARG, "mailbox: open before prepare");
  for (int r = 0; r < m->dev.P; ++r)
    m->dev.peer[r] = r == m->dev.me ? m->dev.local
                                    : static_cast<u64 *>(m->mem.open_peer(handles + (size_t)r * HIP_IPC_HANDLE_SIZE));
}

bool mailbox_validate(eig_ctx_t ctx)
{
  MailboxHost *m = ctx->mbox;
  double *d = ctx->scratch;
  const int P = m->dev.P;
  double v[3] = {(double)(m->dev.me + 1), 1.0, (double)(m->dev.me + 1) * 0.5};
  EIG_HIP(hipMemcpy(d, v, sizeof(v), hipMemcpyHostToDevice));
  launch_mailbox_allreduce(d, 3, m->dev, 200000000ull /* 2 s */, ctx->stream);
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  int err = 1;
  EIG_HIP(hipMemcpy(v, d, sizeof(v), hipMemcpyDeviceToHost));
  EIG_HIP(hipMemcpy(&err, m->dev.err, sizeof(int), hipMemcpyDeviceToHost));
  const double want = 0.5 * P * (P + 1);
  return err == 0 && v[0] == want && v[1] == (double)P && v[2] == 0.5 * want;
}

// Sum `vals` (count doubles) over the mailbox-only ranks, synchronously on ctx->stream; throws when
// the mailbox timed out.  Also a barrier: no rank returns before every rank has published.
void mailbox_sum_sync(eig_ctx_t ctx, std::vector<double> &vals, const char *what)
{
  double *d = dev_alloc<double>(vals.size());
  EIG_HIP(hipMemcpy(d, vals.data(), vals.size() * sizeof(double), hipMemcpyHostToDevice));
  mailbox_sum(ctx, d, (i64)vals.size(), ctx->stream);
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  EIG_HIP(hipMemcpy(vals.data(), d, vals.size() * sizeof(double), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  int err = 0;
  EIG_HIP(hipMemcpy(&err, ctx->mbox->dev.err, sizeof(int), hipMemcpyDeviceToHost));
  EIG_CHECK(err == 0, EIG_ERR_RCCL, std::string(what) + ": mailbox timed out");
}

// (Re)build the halo mailbox with slots of `cap` doubles.  Collective over the mailbox-only ranks,
// which all call it with the same cap (halo_staging_ensure computes it from every rank's plan):
// the old staging is released once every rank is quiet, the new one exported and its IPC handle
// gathered through the mailbox allreduce (each 16-bit chunk one exact double).
// a graph captured before a rebuild keeps the old staging's pointers.
void halobox_setup(eig_ctx_t ctx, i64 cap)
{
  MailboxHost *m = ctx->mbox;
  const int P = m->dev.P, me = m->dev.me;
  constexpr int kChunks = HIP_IPC_HANDLE_SIZE / 2;
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  EIG_HIP(hipStreamSynchronize(ctx->comm_stream));
  std::vector<double> bar(1, 0.0);
  mailbox_sum_sync(ctx, bar, "halo mailbox");  // every rank's exchanges have completed
  halobox_free(ctx);
  auto *h = new HaloBoxHost();
  ctx->hbox = h;
  const size_t fbytes = (size_t)2 * P * kHaloFlagStride * sizeof(u64);
  std::vector<double> g((size_t)P * (kChunks + 1), 0.0);
  unsigned char raw[HIP_IPC_HANDLE_SIZE];
  bool ok = succeeds([&] {
    // the lines, then [2][P][cap] doubles; state: seq[16] at 0, the push / pull tickets at 128 / 256
    h->mem.alloc(fbytes + (size_t)2 * P * (size_t)cap * sizeof(double), 512);
    h->mem.export_handle(raw);
    for (int c = 0; c < kChunks; ++c) g[(size_t)me * (kChunks + 1) + c] = raw[2 * c] + 256.0 * raw[2 * c + 1];
    g[(size_t)me * (kChunks + 1) + kChunks] = 1.0;
  });
  mailbox_sum_sync(ctx, g, "halo mailbox");
  for (int r = 0; r < P; ++r) ok = ok && g[(size_t)r * (kChunks + 1) + kChunks] == 1.0;
  HaloBox &d = h->dev;
  if (ok)
  {
    d.flags = static_cast<u64 *>(h->mem.base);
    d.stage = reinterpret_cast<double *>(static_cast<char *>(h->mem.base) + fbytes);
    d.seq = static_cast<u64 *>(h->mem.state);
    d.ticket = reinterpret_cast<unsigned *>(static_cast<char *>(h->mem.state) + 128);
    d.err = m->dev.err;
    d.cap = cap;
    d.P = P;
    d.me = me;
    ok = succeeds([&] {
      for (int r = 0; r < P; ++r)
      {
        char *base = static_cast<char *>(h->mem.base);
        if (r != me)
        {
          for (int c = 0; c < kChunks; ++c)
          {
            const unsigned v = (unsigned)g[(size_t)r * (kChunks + 1) + c];
            raw[2 * c] = (unsigned char)(v & 255u);
            raw[2 * c + 1] = (unsigned char)(v >> 8);
          }
          base = static_cast<char *>(h->mem.open_peer(raw));
        }
        d.peer_flags[r] = reinterpret_cast<u64 *>(base);
        d.peer_stage[r] = reinterpret_cast<double *>(base + fbytes);
      }
    });
  }
  std::vector<double> agree(1, ok ? 1.0 : 0.0);
  mailbox_sum_sync(ctx, agree, "halo mailbox");
  if (agree[0] != (double)P)
  {
    halobox_free(ctx);
    throw Error(EIG_ERR_RCCL, "halo mailbox: staging setup failed on some rank");
  }
}

// RCCL-agreed minimum of a per-rank flag (every rank takes the same branch afterwards).
bool all_ranks(eig_ctx_t ctx, bool mine)
{
  int *d = dev_alloc<int>(1);
  const int v = mine ? 1 : 0;
  EIG_HIP(hipMemcpy(d, &v, sizeof(int), hipMemcpyHostToDevice));
  EIG_NCCL(ncclAllReduce(d, d, 1, ncclInt32, ncclMin, ctx->comm, ctx->stream));
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  int r = 0;
  EIG_HIP(hipMemcpy(&r, d, sizeof(int), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  return r == 1;
}

// Mailbox allreduce next to the RCCL communicator; each stage is agreed by all ranks, so a rank
// whose export, mapping or validation fails makes every rank stay on ncclAllReduce.
void mailbox_setup_rccl(eig_ctx_t ctx)
{
  const int P = ctx->nranks, me = ctx->rank;
  // (one rank with EIG_COMM_ALWAYS: the one-GPU rehearsal of the mailbox transports)
  const bool want = (P > 1 || ctx->comm_always) && P <= kMaxMailboxRanks;
  if (!all_ranks(ctx, want)) return;
  std::vector<unsigned char> h((size_t)P * HIP_IPC_HANDLE_SIZE, 0);
  bool ok = succeeds([&] { mailbox_prepare(ctx, P, me, h.data() + (size_t)me * HIP_IPC_HANDLE_SIZE); });
  if (!all_ranks(ctx, ok)) return mailbox_free(ctx);
  unsigned char *d = dev_alloc<unsigned char>(h.size());
  EIG_HIP(hipMemcpy(d + (size_t)me * HIP_IPC_HANDLE_SIZE, h.data() + (size_t)me * HIP_IPC_HANDLE_SIZE,
                    HIP_IPC_HANDLE_SIZE, hipMemcpyHostToDevice));
  EIG_NCCL(ncclAllGather(d + (size_t)me * HIP_IPC_HANDLE_SIZE, d, HIP_IPC_HANDLE_SIZE, ncclChar, ctx->comm,
                         ctx->stream));
  EIG_HIP(hipStreamSynchronize(ctx->stream));
  EIG_HIP(hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  ok = succeeds([&] { mailbox_open(ctx, h.data()); });
  if (!all_ranks(ctx, ok)) return mailbox_free(ctx);
  ok = mailbox_validate(ctx);
  if (!all_ranks(ctx, ok)) return mailbox_free(ctx);
  ctx->mbox->ready = true;
}

}  // namespace

void allreduce_sum(eig_ctx_t ctx, double *buf, i64 count, hipStream_t s)
{
  if (!ctx->collectives() || count <= 0) return;
  if (ctx->mailbox_allreduce()) return mailbox_sum(ctx, buf, count, s);
  if (ctx->loop)
  {
    // loopback: every virtual rank publishes its values, then sums all ranks in rank order
    LoopHub &h = *ctx->loop;
    std::vector<double> mine((size_t)count);
    EIG_HIP(hipMemcpyAsync(mine.data(), buf, count * sizeof(double), hipMemcpyDeviceToHost, s));
    EIG_HIP(hipStreamSynchronize(s));
    {
      std::lock_guard<std::mutex> lk(h.m);
      h.red[ctx->rank] = mine;
    }
    h.barrier();
    std::vector<double> tot((size_t)count, 0.0);
    for (int r = 0; r < h.P; ++r)
      for (i64 i = 0; i < count; ++i) tot[i] += h.red[r][i];
    h.barrier();
    EIG_HIP(hipMemcpyAsync(buf, tot.data(), count * sizeof(double), hipMemcpyHostToDevice, s));
    EIG_HIP(hipStreamSynchronize(s));
    return;
  }
  EIG_NCCL(ncclAllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, ctx->comm, s));
  ++ctx->n_ar;
}

bool allreduce_overlaps(eig_ctx_t ctx)
{
  const bool ovl = ctx->collectives() && !ctx->loop && (ctx->mailbox_allreduce() || ctx->comm_red);
  // the reduction stream exists only where it is used (every stream takes a hardware queue)
  if (ovl && !ctx->red_stream) EIG_HIP(hipStreamCreateWithFlags(&ctx->red_stream, hipStreamNonBlocking));
  return ovl;
}

void allreduce_sum_red(eig_ctx_t ctx, double *buf, i64 count, hipStream_t s)
{
  EIG_CHECK(allreduce_overlaps(ctx), EIG_ERR_ARG, "allreduce_sum_red: no concurrent allreduce transport");
  if (ctx->mailbox_allreduce()) return allreduce_sum(ctx, buf, count, s);
  EIG_NCCL(ncclAllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, ctx->comm_red, s));
  ++ctx->n_ar_red;
}

// the capacity comes from this matrix's plan alone; a failed setup forgets earlier matrices.
void halo_staging_ensure(eig_ctx_t ctx, const std::vector<i64> &all, int bc)
{
  const int P = ctx->nranks;
  if (ctx->loop || P <= 1 || !ctx->mailbox_ready()) return;
  // the halo mailbox's slots hold the largest range of any rank's plan, 8 columns wide
  // (subspace.cpp halo_mv exchanges blocks of 8); grown collectively when a matrix needs more
  i64 most = 0;
  std::vector<int64_t> qr(3 * (size_t)P), qs(3 * (size_t)P);
  for (int q = 0; q < P; ++q)
  {
    int nq = 0, ns = 0;
    int rc = eig_plan_halo(P, q, all.data(), bc, 0, qr.data(), &nq, qs.data(), &ns);
    EIG_CHECK(rc == EIG_OK, rc, "eig_plan_halo failed");
    for (int k = 0; k < nq; ++k) most = std::max<i64>(most, qr[3 * k + 2]);
  }
  const i64 cap = 8 * most;
  if (cap <= 0 || (ctx->hbox && ctx->hbox->dev.cap >= cap)) return;
  if (!ctx->comm) return halobox_setup(ctx, cap);  // mailbox-only ranks: their only halo transport
  // beside RCCL the halo mailbox is an option (eig_comm_select_halo): a rank set that could
  // not build it keeps ncclSend / ncclRecv (the failure is agreed inside halobox_setup)
  if (!succeeds([&] { halobox_setup(ctx, cap); }))
  {
    halobox_free(ctx);
    ctx->halo_mailbox = false;
  }
}

// Exchange the ghost entries of the window-layout vector x.  Runs on stream s.
// a timed-out halo mailbox exchange sets the mailbox's error word, which nothing here reads.
void halo_exchange(const eig_mat_s &A, double *x, hipStream_t s, double *x2, int width)
{
  eig_ctx_t ctx = A.ctx;
  if (!ctx->distributed()) return;
  const i64 w = width;
  if (ctx->loop)
  {
    // loopback: publish (x, window begin), then pull every recv range from the owner's vector
    LoopHub &h = *ctx->loop;
    EIG_HIP(hipStreamSynchronize(s));
    {
      std::lock_guard<std::mutex> lk(h.m);
      h.xptr[ctx->rank] = x;
      h.win_begin[ctx->rank] = A.win_begin;
    }
    h.barrier();
    for (const auto &r : A.recvs)
    {
      const i64 global = A.win_begin + r.offset;
      const double *src = h.xptr[r.peer] + (global - h.win_begin[r.peer]) * w;
      EIG_HIP(hipMemcpyAsync(x + r.offset * w, src, r.count * w * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    EIG_HIP(hipStreamSynchronize(s));
    h.barrier();
    if (x2) halo_exchange(A, x2, s, nullptr, width);
    return;
  }
  if (A.sends.empty() && A.recvs.empty()) return;
  if ((!ctx->comm || ctx->halo_mailbox) && ctx->mailbox_ready())
  {
    // mailbox-only ranks, or EIG_HALO_MAILBOX: the xGMI halo mailbox (k_comm.hip).  Every rank of the partition takes part
    // in every exchange of the matrix (an empty side still publishes and waits for its lines).
    HaloXfer snd, rcv, syn;
    auto fill = [&](HaloXfer &side, const std::vector<HaloRange> &ranges) {
      for (const auto &r : ranges)
      {
        side.peer[side.n] = r.peer;
        side.off[side.n] = r.offset;
        side.cnt[side.n++] = r.count;
        if (std::find(syn.peer, syn.peer + syn.n, r.peer) == syn.peer + syn.n) syn.peer[syn.n++] = r.peer;
      }
    };
    fill(snd, A.sends);
    fill(rcv, A.recvs);
    EIG_CHECK(ctx->hbox, EIG_ERR_ARG, "halo exchange: no halo mailbox (matrix created before the mailbox was reopened)");
    launch_halo_mailbox(ctx->hbox->dev, snd, rcv, syn, x, x2, width, s);
  }
  else
  {
    EIG_CHECK(ctx->comm, EIG_ERR_ARG, "halo exchange needs RCCL, the mailbox or the loopback transport");
    EIG_NCCL(ncclGroupStart());
    // per peer, x then x2 on both sides: point-to-point operations match in issue order
    for (const auto &r : A.recvs)
      for (double *v : {x, x2})
        if (v) EIG_NCCL(ncclRecv(v + r.offset * w, (size_t)(r.count * w), ncclDouble, r.peer, ctx->comm, s));
    for (const auto &r : A.sends)
      for (double *v : {x, x2})
        if (v) EIG_NCCL(ncclSend(v + r.offset * w, (size_t)(r.count * w), ncclDouble, r.peer, ctx->comm, s));
    EIG_NCCL(ncclGroupEnd());
  }
  ++ctx->n_halo;
  ctx->n_p2p += (long long)(A.recvs.size() + A.sends.size()) * (x2 ? 2 : 1);
}

std::vector<i64> allgather_rows(eig_ctx_t ctx, const std::vector<i64> &mine)
{
  const int P = ctx->nranks, me = ctx->rank;
  std::vector<i64> all(4 * (size_t)P, 0);
  if (ctx->loop && P > 1)
  {
    LoopHub &h = *ctx->loop;
    {
      std::lock_guard<std::mutex> lk(h.m);
      for (int t = 0; t < 4; ++t) h.gather[4 * me + t] = mine[t];
    }
    h.barrier();
    all = h.gather;
    h.barrier();
  }
  else if (!ctx->comm && P > 1 && ctx->mailbox_ready())
  {
    // mailbox-only ranks (eig_comm_ipc_open): an allgather as an allreduce of zero-padded rows
    // (integers below 2^53: the double sums are exact)
    std::vector<double> g(4 * (size_t)P, 0.0);
    for (int t = 0; t < 4; ++t) g[4 * me + t] = (double)mine[t];
    mailbox_sum_sync(ctx, g, "eig_mat_create_bcsr_dist");
    for (size_t t = 0; t < g.size(); ++t) all[t] = (i64)g[t];
  }
  else if (ctx->comm && P > 1)
  {
    i64 *d = dev_alloc<i64>(4 * (size_t)P);
    EIG_HIP(hipMemcpy(d + 4 * me, mine.data(), 4 * sizeof(i64), hipMemcpyHostToDevice));
    EIG_NCCL(ncclAllGather(d + 4 * me, d, 4 * sizeof(i64), ncclChar, ctx->comm, ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->stream));
    EIG_HIP(hipMemcpy(all.data(), d, 4 * P * sizeof(i64), hipMemcpyDeviceToHost));
    (void)hipFree(d);
  }
  else
    all = mine;
  return all;
}

void comm_destroy(eig_ctx_t ctx)
{
  mailbox_free(ctx);
  if (ctx->comm_red) (void)ncclCommDestroy(ctx->comm_red);
  if (ctx->comm) (void)ncclCommDestroy(ctx->comm);
  ctx->loop = nullptr;  // the hub is owned by eig_loopback_create / _destroy
}

}  // namespace eigmi

// ============================================================================================
// communicator
// ============================================================================================
extern "C" int eig_comm_unique_id(unsigned char id[128])
{
  return guard(nullptr, [&] {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId u;
    EIG_NCCL(ncclGetUniqueId(&u));
    std::memcpy(id, &u, 128);
  });
}


extern "C" int eig_comm_init(eig_ctx_t ctx, int nranks, int rank, const unsigned char id[128])
{
  return eig_comm_init_ex(ctx, nranks, rank, id, 0);
}

extern "C" int eig_comm_init_ex(eig_ctx_t ctx, int nranks, int rank, const unsigned char id[128], int flags)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && id && nranks >= 1 && rank >= 0 && rank < nranks, EIG_ERR_ARG, "eig_comm_init: bad arguments");
    EIG_CHECK((flags & ~(EIG_COMM_MAILBOX | EIG_COMM_ALWAYS)) == 0, EIG_ERR_ARG, "eig_comm_init_ex: unknown flag");
    EIG_CHECK(!ctx->loop && !ctx->mbox, EIG_ERR_ARG, "context already has a transport");
    DeviceGuard dg(ctx->device);
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    EIG_NCCL(ncclCommInitRank(&ctx->comm, nranks, u, rank));
    ctx->nranks = nranks;
    ctx->rank = rank;
    ctx->comm_always = (flags & EIG_COMM_ALWAYS) != 0;
    // second communicator (same ranks, same order) for allreduces that overlap the halo exchange.
    // A rank whose split fails makes every rank drop it (all_ranks), so all ranks agree on
    // allreduce_overlaps() and run the pipelined step's allreduce on the same communicator.
    if (nranks > 1 || ctx->comm_always)
    {
      if (ncclCommSplit(ctx->comm, 0, rank, &ctx->comm_red, nullptr) != ncclSuccess) ctx->comm_red = nullptr;
      if (!all_ranks(ctx, ctx->comm_red != nullptr) && ctx->comm_red)
      {
        (void)ncclCommDestroy(ctx->comm_red);
        ctx->comm_red = nullptr;
      }
    }
    // the mailbox allreduce only on request: set up, validated and agreed by all ranks (else RCCL)
    if (flags & EIG_COMM_MAILBOX) mailbox_setup_rccl(ctx);
  });
}

extern "C" int eig_comm_ipc_handle(eig_ctx_t ctx, int nranks, int rank, unsigned char handle[EIG_IPC_HANDLE_BYTES])
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && handle, EIG_ERR_ARG, "eig_comm_ipc_handle: bad arguments");
    EIG_CHECK(!ctx->comm && !ctx->loop, EIG_ERR_ARG, "context already has a transport");
    DeviceGuard dg(ctx->device);
    mailbox_prepare(ctx, nranks, rank, handle);
  });
}

extern "C" int eig_comm_ipc_open(eig_ctx_t ctx, const unsigned char *handles)
{
  return eig_comm_ipc_open_ex(ctx, handles, 0);
}

extern "C" int eig_comm_ipc_open_ex(eig_ctx_t ctx, const unsigned char *handles, int flags)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && handles && ctx->mbox && !ctx->mbox->ready, EIG_ERR_ARG,
              "eig_comm_ipc_open: call eig_comm_ipc_handle first");
    EIG_CHECK((flags & ~EIG_COMM_ALWAYS) == 0, EIG_ERR_ARG, "eig_comm_ipc_open_ex: unknown flag");
    DeviceGuard dg(ctx->device);
    mailbox_open(ctx, handles);
    ctx->nranks = ctx->mbox->dev.P;
    ctx->rank = ctx->mbox->dev.me;
    ctx->mbox->ready = true;
    ctx->comm_always = (flags & EIG_COMM_ALWAYS) != 0;
  });
}

// the restart zeroes the mailbox, not the halo mailbox's sequence words and flag lines.
extern "C" int eig_comm_select_allreduce(eig_ctx_t ctx, int kind)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && (kind == EIG_AR_RCCL || kind == EIG_AR_MAILBOX || kind == EIG_AR_MAILBOX_STEP), EIG_ERR_ARG,
              "eig_comm_select_allreduce: EIG_AR_RCCL, EIG_AR_MAILBOX or EIG_AR_MAILBOX_STEP");
    EIG_CHECK(kind == EIG_AR_RCCL ? ctx->comm != nullptr : ctx->mailbox_ready(), EIG_ERR_ARG,
              "eig_comm_select_allreduce: that transport is not set up on this context");
    if (ctx->mbox)
    {
      DeviceGuard dg(ctx->device);
      MailboxHost *m = ctx->mbox;
      EIG_HIP(hipStreamSynchronize(ctx->stream));
      if (ctx->comm || ctx->loop)
      {
        // a new selection restarts the mailbox on every rank: after a timed-out call the
        // ranks' sequence words disagree (a lagging rank could match a peer's OLD publication), so
        // with the ranks quiet (barrier over RCCL / the loopback hub), each zeroes its mailbox, its
        // call counters and its error word, and a second barrier keeps any rank from publishing
        // into a mailbox that is not yet zeroed
        m->on = false;
        stream_barrier(ctx);
        EIG_HIP(hipMemsetAsync(m->mem.base, 0, m->mem.bytes, ctx->stream));
        EIG_HIP(hipMemsetAsync(m->mem.state, 0, 256, ctx->stream));
        EIG_HIP(hipStreamSynchronize(ctx->stream));
        stream_barrier(ctx);
      }
      else
      {
        // mailbox alone (eig_comm_ipc_open, no other transport to agree on a restart): only the
        // error word is cleared; after a timeout re-open the mailbox (eig_comm_ipc_handle / _open)
        EIG_HIP(hipMemset(m->dev.err, 0, sizeof(int)));
      }
      m->on = kind != EIG_AR_RCCL;
      m->step = kind == EIG_AR_MAILBOX_STEP;
    }
  });
}

extern "C" int eig_comm_select_halo(eig_ctx_t ctx, int kind)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && (kind == EIG_HALO_RCCL || kind == EIG_HALO_MAILBOX), EIG_ERR_ARG,
              "eig_comm_select_halo: EIG_HALO_RCCL or EIG_HALO_MAILBOX");
    EIG_CHECK(ctx->comm && ctx->mailbox_ready(), EIG_ERR_ARG,
              "eig_comm_select_halo: needs RCCL and a validated mailbox (eig_comm_init_ex EIG_COMM_MAILBOX)");
    EIG_CHECK(kind == EIG_HALO_RCCL || ctx->hbox || ctx->nranks == 1, EIG_ERR_RCCL,
              "eig_comm_select_halo: no halo mailbox staging (set up by eig_mat_create_bcsr_dist; it failed or no "
              "distributed matrix with a halo exists yet)");
    DeviceGuard dg(ctx->device);
    EIG_HIP(hipStreamSynchronize(ctx->stream));
    EIG_HIP(hipStreamSynchronize(ctx->comm_stream));
    ctx->halo_mailbox = kind == EIG_HALO_MAILBOX;
  });
}

extern "C" int eig_comm_info(eig_ctx_t ctx, int *nranks, int *rank, int *allreduce, int *mailbox_errors)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    if (nranks) *nranks = ctx->nranks;
    if (rank) *rank = ctx->rank;
    if (allreduce)
      *allreduce = !ctx->collectives()       ? EIG_AR_NONE
                   : ctx->step_exchange()    ? EIG_AR_MAILBOX_STEP
                   : ctx->mailbox_allreduce() ? EIG_AR_MAILBOX
                   : ctx->loop               ? EIG_AR_LOOPBACK
                                             : EIG_AR_RCCL;
    if (mailbox_errors)
    {
      *mailbox_errors = 0;
      if (ctx->mailbox_ready())
      {
        DeviceGuard dg(ctx->device);
        EIG_HIP(hipStreamSynchronize(ctx->stream));
        EIG_HIP(hipMemcpy(mailbox_errors, ctx->mbox->dev.err, sizeof(int), hipMemcpyDeviceToHost));
      }
    }
  });
}

extern "C" int eig_comm_counters(eig_ctx_t ctx, int64_t out[4])
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && out, EIG_ERR_ARG, "eig_comm_counters: null argument");
    out[0] = ctx->n_ar;
    out[1] = ctx->n_ar_red;
    out[2] = ctx->n_halo;
    out[3] = ctx->n_p2p;
  });
}

extern "C" int eig_loopback_create(int nranks, void **hub)
{
  return guard(nullptr, [&] {
    EIG_CHECK(hub && nranks >= 1, EIG_ERR_ARG, "eig_loopback_create: bad arguments");
    *hub = new LoopHub(nranks);
  });
}

extern "C" int eig_loopback_destroy(void *hub)
{
  delete static_cast<LoopHub *>(hub);
  return EIG_OK;
}

extern "C" int eig_comm_init_loopback(eig_ctx_t ctx, void *hub, int rank)
{
  return guard(ctx, [&] {
    auto *h = static_cast<LoopHub *>(hub);
    EIG_CHECK(ctx && h && rank >= 0 && rank < h->P, EIG_ERR_ARG, "eig_comm_init_loopback: bad arguments");
    EIG_CHECK(!ctx->comm && !ctx->mbox, EIG_ERR_ARG, "context already has a transport");
    ctx->loop = h;
    ctx->nranks = h->P;
    ctx->rank = rank;
  });
}

extern "C" int eig_comm_loopback_mailbox(eig_ctx_t ctx)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && ctx->loop && !ctx->mbox, EIG_ERR_ARG, "eig_comm_loopback_mailbox: loopback rank without a mailbox");
    DeviceGuard dg(ctx->device);
    LoopHub &h = *ctx->loop;
    const int P = h.P, me = ctx->rank;
    unsigned char handle[HIP_IPC_HANDLE_SIZE];
    bool ok = succeeds([&] { mailbox_prepare(ctx, P, me, handle); });
    {
      std::lock_guard<std::mutex> lk(h.m);
      h.mbox[me] = ok ? ctx->mbox->dev.local : nullptr;
      h.flag[me] = ok ? 1 : 0;
    }
    h.barrier();
    for (int r = 0; r < P; ++r) ok = ok && h.flag[r] && h.mbox[r];
    // the virtual ranks share one process and device: the peers' mailboxes are plain device pointers
    if (ok)
      for (int r = 0; r < P; ++r) ctx->mbox->dev.peer[r] = h.mbox[r];
    h.barrier();
    if (ok) ok = mailbox_validate(ctx);  // (every rank's kernel runs concurrently: one queue each)
    {
      std::lock_guard<std::mutex> lk(h.m);
      h.flag[me] = ok ? 1 : 0;
    }
    h.barrier();
    for (int r = 0; r < P; ++r) ok = ok && h.flag[r];
    h.barrier();
    if (!ok)
    {
      mailbox_free(ctx);
      throw Error(EIG_ERR_RCCL, "eig_comm_loopback_mailbox: mailbox setup or validation failed on some rank");
    }
    ctx->mbox->ready = true;
  });
}

extern "C" int eig_comm_allreduce_sum(eig_ctx_t ctx, double *buf, int64_t count)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx && buf && count >= 0, EIG_ERR_ARG, "eig_comm_allreduce_sum: bad arguments");
    allreduce_sum(ctx, buf, count, ctx->stream);
  });
}

extern "C" int eig_comm_barrier(eig_ctx_t ctx)
{
  return guard(ctx, [&] {
    EIG_CHECK(ctx, EIG_ERR_ARG, "null context");
    stream_barrier(ctx);
  });
}
