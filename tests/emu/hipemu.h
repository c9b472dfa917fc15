// hipemu.h -- TEST-ONLY CPU emulation of the tiny HIP subset the engine uses.
//
// Purpose: this build container has no GPU.  Compiling fourier_amd/csrc/engine.cpp with
// `g++ -DFOURIER_EMU -include tests/emu/hipemu.h` runs the *same* kernel source on the CPU
// (one fiber per GPU thread, __syncthreads() = yield), so kernel index arithmetic,
// plan logic and the C-ABI are checked before any GPU minute is spent.  It also counts LDS
// bank conflicts (see lds_trace below).
//
// This is NOT a product path and NOT a fallback: it lives under tests/, is built only by
// tests/emu/build_emu.py, and the product package (fourier_amd) never loads it.
#pragma once

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#ifndef __restrict__
#define __restrict__ __restrict
#endif

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

typedef int hipError_t;
typedef void* hipStream_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2, hipErrorNotReady = 600 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };

namespace hipemu {
struct Tls {
  dim3 tid, bid, bdim, gdim;
  unsigned char* smem = nullptr;
  int* shfl = nullptr;  // one slot per thread of the block: cross-lane shuffles
  void** sched = nullptr;  // where the scheduler's stack pointer is parked while a fiber runs
  void** self = nullptr;   // where the running fiber's stack pointer is parked while it waits
  int why = 0;             // why the running fiber yielded: 0 a block barrier, 1 a wave shuffle (Schedule below)
};
inline Tls& tls() {
  static thread_local Tls t;
  return t;
}

// ---- LDS access tracing (bank-conflict model from MI355X_MICROARCH.md, LDS table) ----
struct LdsStats {
  std::atomic<uint64_t> instr{0}, cycles{0}, ideal{0};
};
inline LdsStats& lds_stats() { static LdsStats s; return s; }
struct LdsAccess { uint32_t addr; uint16_t bytes; uint8_t is_write; uint32_t site; };
inline std::vector<LdsAccess>& lds_log() { static thread_local std::vector<LdsAccess> v; return v; }
inline bool& lds_trace_on() { static bool on = getenv("HIPEMU_LDS_TRACE") != nullptr; return on; }
inline void lds_note(const void* p, unsigned bytes, bool is_write, uint32_t site) {
  if (!lds_trace_on()) return;
  Tls& t = tls();
  const size_t off = (size_t)((const unsigned char*)p - t.smem);
  if (off >= ((size_t)1 << 20)) return;  // not an LDS address: a pass that reads its input straight from global memory (mix_gio)
  lds_log().push_back({(uint32_t)off, (uint16_t)bytes, (uint8_t)is_write, site});
}

// cost (LDS-array cycles) of one wave-instruction given 64 lane byte-addresses
inline unsigned lds_cost(const uint32_t* addr, int nl, unsigned bytes, bool is_write, unsigned* ideal) {
  // lane groups and bank modulus per MI355X_MICROARCH.md (LDS section)
  std::vector<std::vector<int>> groups;
  unsigned modulus = 32;
  auto contiguous = [&](int gsz) {
    for (int g = 0; g < 64; g += gsz) { std::vector<int> v; for (int l = g; l < g + gsz; ++l) v.push_back(l); groups.push_back(v); }
  };
  if (!is_write) {
    if (bytes <= 4) { contiguous(32); modulus = 32; }
    else if (bytes == 8) { contiguous(32); modulus = 64; }
    else {  // b128: four non-contiguous 16-lane groups
      modulus = 64;
      groups = {{0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27}, {4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31},
                {32,33,34,35,44,45,46,47,52,53,54,55,56,57,58,59}, {36,37,38,39,40,41,42,43,48,49,50,51,60,61,62,63}};
    }
  } else {
    modulus = 32;
    if (bytes <= 4) contiguous(32); else if (bytes == 8) contiguous(16); else contiguous(8);
  }
  unsigned total = 0;
  *ideal = (unsigned)groups.size();
  for (auto& g : groups) {
    std::map<unsigned, std::vector<uint32_t>> bank2addrs;
    for (int l : g) {
      if (l >= nl || addr[l] == 0xffffffffu) continue;  // (0xffffffff: the lane is masked off in this instruction)
      for (unsigned d = 0; d < bytes / 4 + (bytes < 4); ++d) {
        uint32_t dw = addr[l] / 4 + d;
        auto& v = bank2addrs[dw % modulus];
        if (std::find(v.begin(), v.end(), dw) == v.end()) v.push_back(dw);
      }
    }
    unsigned worst = 1;
    for (auto& kv : bank2addrs) worst = std::max<unsigned>(worst, (unsigned)kv.second.size());
    total += worst;
  }
  return total;
}

inline unsigned char* smem() { return tls().smem; }

// Fiber switch without a system call (swapcontext saves and restores the signal mask: two rt_sigprocmask calls per
// switch, and a barrier of a 1024-thread block is 1024 switches -- the CPU test suite spent more time in the kernel than
// in the emulated kernels).  x86-64 System V: the callee-saved registers and the stack pointer are the whole context.
#if !defined(__x86_64__)
#error "tests/emu/hipemu.h: the fiber switch is written for x86-64"
#endif
extern "C" {
__attribute__((naked, noinline, used)) static void hipemu_switch(void** /*save_sp: rdi*/, void* /*load_sp: rsi*/) {
  asm volatile(
      "pushq %rbp\n\tpushq %rbx\n\tpushq %r12\n\tpushq %r13\n\tpushq %r14\n\tpushq %r15\n\t"
      "movq %rsp, (%rdi)\n\t"
      "movq %rsi, %rsp\n\t"
      "popq %r15\n\tpopq %r14\n\tpopq %r13\n\tpopq %r12\n\tpopq %rbx\n\tpopq %rbp\n\t"
      "ret\n\t");
}
}

inline void syncthreads() {
  Tls& t = tls();
  t.why = 0;
  hipemu_switch(t.self, *t.sched);
}
// a wave-level rendezvous (the two halves of __shfl_xor).  Under the default schedule the scheduler does not look at `why`: the
// shuffle is two whole-block barriers, as it always was.
inline void syncwave() {
  Tls& t = tls();
  t.why = 1;
  hipemu_switch(t.self, *t.sched);
}

// ---- schedules: the order in which the threads of a block run between two barriers, and the order in which the blocks run.
// HIPEMU_SCHEDULE="<threads>:<blocks>", read at every launch (tests/schedule_cases.py sets it per run).  Unset, empty or
// "ascending:ascending" is the default, which is exactly what this file always did: threads in ascending order, blocks handed out in
// ascending order to one worker per core, __shfl_xor as two block barriers.
//   threads   ascending | descending | waves-descending (lanes ascending) | permutation-1 | permutation-2
//   blocks    ascending | descending | permutation      (the last two on ONE worker: the order is then the order of execution)
// Every other schedule runs wave by wave: a wave runs on through its shuffles -- which wait for its own 64 lanes only, as on the
// hardware -- to its next block barrier before the next wave starts.  The permutations order the waves and, per wave, the lanes
// (xorshift64* Fisher-Yates from a fixed seed: the same schedule every time).
// What this shows: a hazard between two threads, or two blocks, whose two relative orders are both among the schedules and whose
// stale value differs from the fresh one.  What it cannot show: anything the memory model decides (a missing wait or fence), and
// blocks that must run at the same time (a kernel that waits on other workgroups hangs under a serial block order).
struct Schedule {
  enum Threads { T_ASC, T_DESC, T_WAVES_DESC, T_PERM1, T_PERM2 } threads = T_ASC;
  enum Blocks { B_ASC, B_DESC, B_PERM } blocks = B_ASC;
  bool is_default() const { return threads == T_ASC && blocks == B_ASC; }
};
inline Schedule schedule() {
  Schedule s;
  const char* e = getenv("HIPEMU_SCHEDULE");
  if (!e || !*e) return s;
  const char* colon = strchr(e, ':');
  const std::string th = colon ? std::string(e, colon) : std::string(e), bl = colon ? std::string(colon + 1) : std::string("ascending");
  static const char* const TH[] = {"ascending", "descending", "waves-descending", "permutation-1", "permutation-2"};
  static const char* const BL[] = {"ascending", "descending", "permutation"};
  int ti = -1, bi = -1;
  for (int i = 0; i < 5; ++i) if (th == TH[i]) ti = i;
  for (int i = 0; i < 3; ++i) if (bl == BL[i]) bi = i;
  if (ti < 0 || bi < 0) { fprintf(stderr, "hipemu: HIPEMU_SCHEDULE=%s names no schedule\n", e); abort(); }  // a typo must not pass as the default
  s.threads = (Schedule::Threads)ti;
  s.blocks = (Schedule::Blocks)bi;
  return s;
}
inline void permute(std::vector<unsigned>& v, uint64_t seed) {
  uint64_t x = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
  for (size_t i = v.size(); i > 1; --i) {
    x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
    std::swap(v[i - 1], v[(size_t)((x * 0x2545F4914F6CDD1Dull) >> 33) % i]);
  }
}
// the order of the waves of a block and, flattened wave after wave, of each wave's lanes (thread indices)
inline void thread_order(Schedule::Threads how, unsigned nthreads, std::vector<unsigned>& waves, std::vector<unsigned>& lanes) {
  const unsigned nw = (nthreads + 63) / 64;
  waves.resize(nw);
  lanes.resize(nthreads);
  for (unsigned w = 0; w < nw; ++w) waves[w] = w;
  for (unsigned i = 0; i < nthreads; ++i) lanes[i] = i;
  const uint64_t seed = how == Schedule::T_PERM1 ? 1 : 2;
  if (how == Schedule::T_DESC || how == Schedule::T_WAVES_DESC) std::reverse(waves.begin(), waves.end());
  if (how == Schedule::T_PERM1 || how == Schedule::T_PERM2) permute(waves, seed);
  for (unsigned w = 0; w < nw; ++w) {
    const unsigned lo = w * 64, hi = std::min(nthreads, lo + 64);
    if (how == Schedule::T_DESC) std::reverse(lanes.begin() + lo, lanes.begin() + hi);
    if (how == Schedule::T_PERM1 || how == Schedule::T_PERM2) {
      std::vector<unsigned> v(lanes.begin() + lo, lanes.begin() + hi);
      permute(v, seed * 1000003u + w + 17);
      std::copy(v.begin(), v.end(), lanes.begin() + lo);
    }
  }
}

struct FiberArg {
  std::function<void()>* body;
  bool done;
};
extern "C" {
__attribute__((noinline, used)) static void hipemu_fiber_main(FiberArg* fa) {
  (*fa->body)();
  fa->done = true;
  for (;;) {  // a finished fiber is never resumed; park it
    Tls& t = tls();
    hipemu_switch(t.self, *t.sched);
  }
}
// first activation of a fiber: hipemu_switch "returns" here with the FiberArg in r12 (see fiber_prepare)
__attribute__((naked, noinline, used)) static void hipemu_trampoline() {
  asm volatile("movq %r12, %rdi\n\tcallq hipemu_fiber_main\n\tud2\n\t");
}
}
// lay out a fresh stack so that the first hipemu_switch into it pops the callee-saved registers (r12 = the argument) and
// returns into the trampoline with a 16-byte aligned stack pointer
// Fiber stacks come from a pool that outlives the launches: a value-initialised vector of nthreads * 128 KiB per worker
// and launch was a 128 MiB memset (and as many page faults) each time.
struct StackPool {
  static std::mutex& mu() { static std::mutex m; return m; }
  static std::vector<std::pair<unsigned char*, size_t>>& free_list() { static std::vector<std::pair<unsigned char*, size_t>> v; return v; }
  struct Lease {
    unsigned char* p = nullptr;
    size_t bytes = 0;
    explicit Lease(size_t need) {
      {
        std::lock_guard<std::mutex> g(mu());
        auto& fl = free_list();
        for (size_t i = 0; i < fl.size(); ++i)
          if (fl[i].second >= need) { p = fl[i].first; bytes = fl[i].second; fl.erase(fl.begin() + (long)i); break; }
      }
      if (!p) { p = (unsigned char*)malloc(need); bytes = need; }
      if (!p) { fprintf(stderr, "hipemu: out of memory for fiber stacks\n"); abort(); }
    }
    ~Lease() {
      std::lock_guard<std::mutex> g(mu());
      free_list().push_back({p, bytes});
    }
    unsigned char* data() const { return p; }
  };
};

inline void* fiber_prepare(unsigned char* stack, size_t bytes, FiberArg* fa) {
  uintptr_t top = ((uintptr_t)(stack + bytes)) & ~(uintptr_t)15;
  void** sp = (void**)(top - 16 - 56);
  sp[0] = nullptr;                       // r15
  sp[1] = nullptr;                       // r14
  sp[2] = nullptr;                       // r13
  sp[3] = (void*)fa;                     // r12
  sp[4] = nullptr;                       // rbx
  sp[5] = nullptr;                       // rbp
  sp[6] = (void*)&hipemu_trampoline;     // return address
  return (void*)sp;
}

template <typename K, typename A>
void launch(dim3 grid, dim3 block, size_t smem_bytes, K kernel, A arg) {
  const unsigned nblocks = grid.x * grid.y * grid.z;
  const unsigned nthreads = block.x * block.y * block.z;
  unsigned nworkers = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), nblocks);
  if (getenv("HIPEMU_THREADS")) nworkers = std::min<unsigned>(nworkers, (unsigned)atoi(getenv("HIPEMU_THREADS")));
  if (lds_trace_on()) nworkers = 1;
  const Schedule sch = lds_trace_on() ? Schedule() : schedule();  // (the LDS trace models the default order)
  std::vector<unsigned> block_order, wave_order, lane_order;
  if (sch.blocks != Schedule::B_ASC) {  // one worker: the order below is the order of execution
    nworkers = 1;
    block_order.resize(nblocks);
    for (unsigned b = 0; b < nblocks; ++b) block_order[b] = nblocks - 1 - b;
    if (sch.blocks == Schedule::B_PERM) permute(block_order, 3);
  }
  if (!sch.is_default()) thread_order(sch.threads, nthreads, wave_order, lane_order);
  std::atomic<unsigned> next{0};
  auto worker = [&]() {
    const size_t STACK = 128 * 1024;
    StackPool::Lease stacks((size_t)nthreads * STACK);  // reused across launches: no zeroing, no fresh page faults
    std::vector<void*> ctx(nthreads);  // parked stack pointers of the fibers
    std::vector<FiberArg> fargs(nthreads);
    std::vector<unsigned char> smem_buf(smem_bytes + 64);
    std::vector<int> shfl_buf(nthreads);
    std::vector<size_t> log_mark(nthreads);
    std::vector<std::vector<LdsAccess>> tlog(nthreads);
    void* sched = nullptr;             // parked stack pointer of this scheduler
    std::function<void()> body = [&]() { kernel(arg); };
    for (;;) {
      unsigned b = next.fetch_add(1);
      if (b >= nblocks) break;
      if (!block_order.empty()) b = block_order[b];
      Tls& t = tls();
      t.bdim = block; t.gdim = grid;
      t.bid = dim3(b % grid.x, (b / grid.x) % grid.y, b / (grid.x * grid.y));
      t.smem = smem_buf.data();
      t.shfl = shfl_buf.data();
      t.sched = &sched;
      std::memset(smem_buf.data(), 0xCD, smem_buf.size());  // poison: catches reads of unwritten LDS
      for (unsigned i = 0; i < nthreads; ++i) {
        fargs[i] = {&body, false};
        ctx[i] = fiber_prepare(stacks.data() + (size_t)i * STACK, STACK, &fargs[i]);
      }
      unsigned remaining = nthreads;
      if (!sch.is_default()) {
        // wave by wave up to the next block barrier; inside a wave, sweeps over its lanes in the schedule's order, each lane
        // running to its next yield.  A sweep that ends with the whole wave at a shuffle releases it; one that ends with part
        // of the wave there is a shuffle some lanes never reach.
        enum : uint8_t { RUN, AT_BARRIER, AT_SHUFFLE, DONE };
        std::vector<uint8_t> state(nthreads, RUN);
        while (remaining) {
          unsigned finished = 0;
          for (unsigned w : wave_order) {
            const unsigned lo = w * 64, hi = std::min(nthreads, lo + 64);
            for (;;) {
              for (unsigned k = lo; k < hi; ++k) {
                const unsigned i = lane_order[k];
                if (state[i] != RUN) continue;
                t.tid = dim3(i % block.x, (i / block.x) % block.y, i / (block.x * block.y));
                t.self = &ctx[i];
                hipemu_switch(&sched, ctx[i]);
                state[i] = fargs[i].done ? DONE : t.why == 1 ? AT_SHUFFLE : AT_BARRIER;
              }
              unsigned shuffling = 0;
              for (unsigned i = lo; i < hi; ++i) shuffling += state[i] == AT_SHUFFLE;
              if (!shuffling) break;
              if (shuffling != hi - lo) {
                fprintf(stderr, "hipemu: divergent __shfl_xor in block %u, wave %u (%u of %u lanes reached it)\n", b, w, shuffling, hi - lo);
                abort();
              }
              for (unsigned i = lo; i < hi; ++i) state[i] = RUN;
            }
            for (unsigned i = lo; i < hi; ++i) finished += state[i] == DONE;
          }
          if (finished != 0 && finished != remaining) {
            fprintf(stderr, "hipemu: divergent __syncthreads() in block %u (%u of %u threads exited)\n", b, finished, remaining);
            abort();
          }
          remaining -= finished;
          for (unsigned i = 0; i < nthreads; ++i) if (state[i] == AT_BARRIER) state[i] = RUN;
        }
      }
      while (remaining) {
        unsigned ran = 0, finished = 0;
        for (unsigned i = 0; i < nthreads; ++i) {
          if (fargs[i].done) continue;
          t.tid = dim3(i % block.x, (i / block.x) % block.y, i / (block.x * block.y));
          t.self = &ctx[i];
          if (lds_trace_on()) lds_log().clear();
          hipemu_switch(&sched, ctx[i]);
          if (lds_trace_on()) tlog[i] = lds_log();
          ++ran;
          if (fargs[i].done) ++finished;
        }
        if (finished != 0 && finished != ran) {
          fprintf(stderr, "hipemu: divergent __syncthreads() in block %u (%u of %u threads exited)\n", b, finished, ran);
          abort();
        }
        remaining -= finished;
        if (lds_trace_on()) {  // between two barriers: k-th access of every lane in a wave = one instruction
          for (unsigned w = 0; w < nthreads; w += 64) {
            unsigned nl = std::min(64u, nthreads - w);
            // (a lane without any access between the two barriers is masked off in these instructions: the stages of kernels_chirpz.h run on
            // part of a wave's lanes)
            unsigned first = nl;
            for (unsigned l = 0; l < nl && first == nl; ++l)
              if (!tlog[w + l].empty()) first = l;
            if (first == nl) continue;
            const unsigned f = w + first;
            size_t na = tlog[f].size();
            for (size_t k = 0; k < na; ++k) {
              uint32_t addr[64] = {0};
              bool ok = true;
              for (unsigned l = 0; l < nl; ++l) {
                if (tlog[w + l].empty()) { addr[l] = 0xffffffffu; continue; }
                if (tlog[w + l].size() != na || tlog[w + l][k].site != tlog[f][k].site) { ok = false; break; }
                addr[l] = tlog[w + l][k].addr;
              }
              if (!ok) continue;
              unsigned ideal;
              unsigned c = lds_cost(addr, (int)nl, tlog[f][k].bytes, tlog[f][k].is_write, &ideal);
              lds_stats().instr++; lds_stats().cycles += c; lds_stats().ideal += ideal;
              if (getenv("HIPEMU_LDS_VERBOSE") && b == 0 && w == 0)
                fprintf(stderr, "lds site %u %s b%u: %u cycles (ideal %u)\n", tlog[f][k].site, tlog[f][k].is_write ? "W" : "R",
                        tlog[f][k].bytes, c, ideal);
            }
          }
          for (auto& v : tlog) v.clear();
        }
      }
    }
  };
  if (nworkers <= 1) { worker(); return; }
  std::vector<std::thread> th;
  for (unsigned i = 0; i < nworkers; ++i) th.emplace_back(worker);
  for (auto& t : th) t.join();
}
}  // namespace hipemu

#define threadIdx (hipemu::tls().tid)
#define blockIdx (hipemu::tls().bid)
#define blockDim (hipemu::tls().bdim)
#define gridDim (hipemu::tls().gdim)
inline void __syncthreads() { hipemu::syncthreads(); }
// wave shuffle: publish, rendezvous, read the partner's slot, rendezvous.  The rendezvous is the wave's own under every schedule but
// the default, where it is the whole block's (hipemu::Schedule)
inline int __shfl_xor(int v, int lane_mask) {
  hipemu::Tls& t = hipemu::tls();
  const unsigned i = t.tid.x + t.bdim.x * (t.tid.y + t.bdim.y * t.tid.z);
  t.shfl[i] = v;
  hipemu::syncwave();
  const int r = t.shfl[(i & ~63u) | ((i ^ (unsigned)lane_mask) & 63u)];
  hipemu::syncwave();
  return r;
}

// ---- device intrinsics used by the XCD-fused kernel (inter-workgroup hand-offs): CPU stand-ins ----
// blocks run concurrently on worker threads, so the atomics are real; seq_cst gives the ordering the GPU protocol
// gets from "stores reached the L2 (vmcnt(0)) -> counter increment" / "counter seen -> sc1 loads"
#define __HIP_MEMORY_SCOPE_AGENT 4
#define __HIP_MEMORY_SCOPE_WORKGROUP 2
#define __hip_atomic_load(p, order, scope) __atomic_load_n((p), __ATOMIC_SEQ_CST)
#define __hip_atomic_store(p, v, order, scope) __atomic_store_n((p), (v), __ATOMIC_SEQ_CST)
#define __hip_atomic_fetch_add(p, v, order, scope) __atomic_fetch_add((p), (v), __ATOMIC_SEQ_CST)
inline void __builtin_amdgcn_s_sleep(int) { std::this_thread::yield(); }
inline uint32_t __builtin_amdgcn_s_getreg(int) {  // HW_REG_XCC_ID: spread the blocks over a few pretend XCDs
  if (const char* e = getenv("HIPEMU_XCDS")) return hipemu::tls().bid.x % (unsigned)atoi(e);
  return hipemu::tls().bid.x % 3;
}
// buffer descriptor: base + byte count; the offset (not the scalar offset) is range-checked dword by dword, as the hardware does
struct __amdgpu_buffer_rsrc_t { unsigned char* base; uint32_t num_records; };
inline __amdgpu_buffer_rsrc_t __builtin_amdgcn_make_buffer_rsrc(void* p, int, int num_records, int) { return {(unsigned char*)p, (uint32_t)num_records}; }
struct hipemu_b128 { uint32_t w[4]; };
inline hipemu_b128 __builtin_amdgcn_raw_buffer_load_b128(__amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  hipemu_b128 v;
  for (int d = 0; d < 4; ++d) {
    const uint64_t o = (uint64_t)(uint32_t)voff + 4u * (unsigned)d;
    if (o + 4 <= r.num_records) memcpy(&v.w[d], r.base + (uint32_t)soff + o, 4); else v.w[d] = 0;
  }
  return v;
}
struct hipemu_b64 { uint32_t w[2]; };
inline hipemu_b64 __builtin_amdgcn_raw_buffer_load_b64(__amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  hipemu_b64 v;
  for (int d = 0; d < 2; ++d) {
    const uint64_t o = (uint64_t)(uint32_t)voff + 4u * (unsigned)d;
    if (o + 4 <= r.num_records) memcpy(&v.w[d], r.base + (uint32_t)soff + o, 4); else v.w[d] = 0;
  }
  return v;
}
inline void __builtin_amdgcn_raw_buffer_store_b64(hipemu_b64 v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  for (int d = 0; d < 2; ++d) {
    const uint64_t o = (uint64_t)(uint32_t)voff + 4u * (unsigned)d;
    if (o + 4 <= r.num_records) memcpy(r.base + (uint32_t)soff + o, &v.w[d], 4);
  }
}
inline void __builtin_amdgcn_raw_buffer_store_b128(hipemu_b128 v, __amdgpu_buffer_rsrc_t r, int voff, int soff, int) {
  for (int d = 0; d < 4; ++d) {
    const uint64_t o = (uint64_t)(uint32_t)voff + 4u * (unsigned)d;
    if (o + 4 <= r.num_records) memcpy(r.base + (uint32_t)soff + o, &v.w[d], 4);
  }
}

// LDS-DMA (buffer_load_dwordx4 ... lds): the destination is a wave-uniform LDS base plus lane * size; 1-D blocks
inline void __builtin_amdgcn_raw_ptr_buffer_load_lds(__amdgpu_buffer_rsrc_t r, void* lds, int size, int voff, int soff, int off, int) {
  const hipemu_b128 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff + off, soff, 0);
  memcpy((unsigned char*)lds + (size_t)(hipemu::tls().tid.x & 63u) * (size_t)size, &v, (size_t)size);
}
inline int __builtin_amdgcn_readfirstlane(int v) { return v; }  // callers pass wave-uniform values
inline void __builtin_amdgcn_s_waitcnt(int) {}

// ---- host API subset ----
namespace hipemu { inline uint64_t& alloc_count() { static uint64_t c = 0; return c; } }
inline hipError_t hipMalloc(void** p, size_t n) {
  hipemu::alloc_count()++;
  if (const char* cap = getenv("HIPEMU_MAX_ALLOC"))  // tests: pretend the device is out of memory above this size
    if (n > (size_t)atoll(cap)) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = n ? malloc(n) : nullptr;
  return (*p || !n) ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
enum { hipHostMallocMapped = 2 };
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return hipMalloc(p, n); }
inline hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memmove(d, s, n); return hipSuccess; }
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
enum { hipStreamNonBlocking = 1, hipEventDisableTiming = 2 };
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = (hipStream_t)malloc(1); return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "hipemu error"; }
#include <chrono>
struct hipemu_event { std::chrono::steady_clock::time_point t; };
typedef hipemu_event* hipEvent_t;
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = new hipemu_event(); return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t e) { delete e; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { e->t = std::chrono::steady_clock::now(); return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = new hipemu_event(); return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  *ms = std::chrono::duration<float, std::milli>(b->t - a->t).count();
  return hipSuccess;
}
template <typename F> inline hipError_t hipFuncSetAttribute(F, hipFuncAttribute, int) { return hipSuccess; }
template <typename F> inline hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, F, int, size_t) { *n = 2; return hipSuccess; }
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount = 63 };
inline hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) { *v = 3; return hipSuccess; }
