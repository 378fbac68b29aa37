// Time-synchronous beam search (espnet BeamSearchTimeSync, the reference's Speech2Text(time_sync=True),
// src/inference/avsr_inference.py:94, 257-275): a CTC prefix beam search walked frame by frame, every prefix that enters the beam
// rescored by the attention decoder and the LM.  The reference is a Python loop over the frames with dictionaries keyed by token tuples,
// one utterance at a time; here one workgroup per utterance does a frame's bookkeeping:
//   * a prefix is a node of a per-utterance trie in device memory (parent, token); node 0 is (<sos>,).  A prefix has ONE node for the
//     whole utterance: an open-addressing table keyed by (parent node, token) finds the node of a prefix that left the beam and comes
//     back, so "lp is another beam member" is the comparison of two integers and two sources of one prefix are never un-merged.
//   * the beam is K slots; a member keeps its slot while it stays, so its scorer rows [K][V] stay where they are.
//   * dp - the prefixes expanded in the previous frame that are not beam members - is a hash table in LDS: key, p_nb, p_b.
//   * a frame's expansion is DENSE: entry i < K is beam member i itself, entry K + j * NC + q is member j extended by candidate q.  The
//     only two entries that can name one prefix are (j, q) and a member i whose parent is j: (j, q) is then folded into i (the merge).
//     Every entry is computed by one thread from the previous frame's state alone (a gather: no atomics on scores).
// tavsr_timesync_step runs one frame (the state image travels through device memory between launches, the scorers run in between),
// tavsr_timesync_search every frame of an utterance in one launch: the same device function, the same bits.
#include "common.h"

namespace tavsr {

constexpr int kTsLdsBytes = 160 * 1024;
constexpr int kTsThreads = 256;
constexpr int kTsRowsMaxKeys = 1024;

// offsets in 4-byte words.  [0, persist): the state image of an utterance (LDS while a kernel runs, the head of the utterance's
// workspace between launches); [persist, ws_words): the trie and its table (device memory only); LDS scratch from `persist` on.
struct TsLay {
  int NC, E, EP, HCAP, NN, GCAP;      // EP: E rounded up to 8 (the ranking loop reads the scores in groups)
  int node, tok, par, depth, pnb, pb, score, dec, lm, order, misc, hkey, hnb, hb, persist;
  int tpar, ttok, gkey, gval, ws_words;
  int p, flag, cand, pl, psl, e_nb, e_b, e_sc, e_dec, e_lm, e_fl, sel, src, lds_words;
};
enum { TS_NBEAM = 0, TS_NNODES = 1, TS_OVERFLOW = 2, TS_NCAND = 3, TS_MISC = 8 };

__host__ __device__ inline int ts_pow2(int64_t n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

__host__ __device__ inline TsLay ts_layout(int K, int V, int T, int C) {
  TsLay o;
  o.NC = 2 * C < V ? 2 * C : V;
  o.E = K + K * o.NC;
  o.EP = (o.E + 7) & ~7;
  o.HCAP = ts_pow2(2 * (int64_t)o.E);
  o.NN = 1 + K * T;
  o.GCAP = ts_pow2(2 * (int64_t)o.NN);
  int w = 0;
  o.node = w; w += K;
  o.tok = w; w += K;
  o.par = w; w += K;
  o.depth = w; w += K;
  o.pnb = w; w += K;
  o.pb = w; w += K;
  o.score = w; w += K;
  o.dec = w; w += K;
  o.lm = w; w += K;
  o.order = w; w += K;
  o.misc = w; w += TS_MISC;
  o.hkey = w; w += o.HCAP;
  o.hnb = w; w += o.HCAP;
  o.hb = w; w += o.HCAP;
  o.persist = w;
  int g = w;
  o.tpar = g; g += o.NN;
  o.ttok = g; g += o.NN;
  o.gkey = g; g += o.GCAP;
  o.gval = g; g += o.GCAP;
  o.ws_words = g;
  o.p = w; w += V;
  o.flag = w; w += V;
  o.cand = w; w += o.NC;
  o.pl = w; w += K;
  o.psl = w; w += K;
  o.e_nb = w; w += o.E;
  o.e_b = w; w += o.E;
  o.e_sc = w; w += o.EP;
  o.e_dec = w; w += o.E;
  o.e_lm = w; w += o.E;
  o.e_fl = w; w += o.E;
  o.sel = w; w += K;
  o.src = w; w += K;
  o.lds_words = w;
  return o;
}

static bool ts_ok(int K, int V, int T, int C) {
  if (K < 1 || K > 64 || V < 2 || V > (1 << 15) || T < 1 || T > (1 << 16) || C < 1 || C > V) return false;
  if (((int64_t)K * T + 3) * V >= ((int64_t)1 << 31)) return false;      // a (parent node, token) key is one int32
  if ((int64_t)K * (2 * (int64_t)C + 1) > (1 << 16)) return false;
  return (int64_t)ts_layout(K, V, T, C).lds_words * 4 <= kTsLdsBytes;
}

struct TsArgs {
  const float* lpz;
  const int64_t* lens;
  int32_t* ws;
  const float* dec_new;
  float* dec_rows;
  const float* lm_new;
  float* lm_rows;
  int64_t* tok;
  int32_t* pos;
  int32_t* nkeys;
  int32_t* anc;
  int32_t* anc_tmp;
  int64_t ld_anc;
  int32_t* frame_dev;
  int U, K, V, T, C, blank, sos;
  float w_ctc, w_dec, w_lm, pen;
};

__device__ inline float ts_lae(float a, float b) {      // logaddexp; (-inf, -inf) -> -inf
  const float m = fmaxf(a, b);
  if (!(m > -INFINITY)) return m;
  return m + log1pf(expf(fminf(a, b) - m));
}

__device__ inline uint32_t ts_hash(int key) { return ((uint32_t)key * 2654435761u) >> 10; }

// one frame of one utterance; L: the state image followed by the scratch.  Enters and leaves behind a workgroup barrier.
__device__ void ts_frame(const TsArgs& a, const TsLay& o, float* L, int u, int t) {
  int* Li = reinterpret_cast<int*>(L);
  const int tid = threadIdx.x, nt = blockDim.x, K = a.K, V = a.V, NC = o.NC, blank = a.blank;
  int32_t* wsu = a.ws + (int64_t)u * o.ws_words;
  // the frame's row, and log p(prefix) of every beam member
  const float* pr = a.lpz + ((int64_t)u * a.T + t) * V;
  for (int c = tid; c < V; c += nt) L[o.p + c] = pr[c];
  for (int k = tid; k < K; k += nt) L[o.pl + k] = Li[o.node + k] >= 0 ? ts_lae(L[o.pnb + k], L[o.pb + k]) : -INFINITY;
  for (int e = tid; e < o.E; e += nt) Li[o.e_fl + e] = 0;
  __syncthreads();
  // 1. candidates: p[c] >= the C-th largest value <=> fewer than C values are larger; ties at the threshold are all kept
  for (int c = tid; c < V; c += nt) {
    const float pc = L[o.p + c];
    int cnt = 0;
    for (int c2 = 0; c2 < V; ++c2) cnt += L[o.p + c2] > pc ? 1 : 0;
    Li[o.flag + c] = cnt < a.C ? 1 : 0;
  }
  __syncthreads();
  if (tid < 64) {      // in token order; more than NC of them (ties): the utterance is flagged, the surplus leaves the flags too
    int n = 0;
    for (int base = 0; base < V; base += 64) {
      const int c = base + tid;
      const bool f = c < V && Li[o.flag + c] != 0;
      const uint64_t m = __ballot(f);
      const int idx = n + __popcll(m & ((1ull << tid) - 1ull));
      if (f) {      // the flag becomes the token's place in the list + 1
        if (idx < NC) Li[o.cand + idx] = c;
        Li[o.flag + c] = idx < NC ? idx + 1 : 0;
      }
      n += __popcll(m);
    }
    if (tid == 0) {
      Li[o.misc + TS_NCAND] = n < NC ? n : NC;
      if (n > NC) Li[o.misc + TS_OVERFLOW] = 1;
    }
  }
  __syncthreads();
  // the merge, found once per member: the slot of its parent (where the parent is a beam member), and - where the member's own token is a
  // candidate - the mark (8) on the entry (parent, token) that IS this member
  for (int i = tid; i < K; i += nt) {
    int pslot = -1;
    if (Li[o.node + i] >= 0 && Li[o.par + i] >= 0) {
      const int par = Li[o.par + i];
      for (int j = 0; j < K; ++j) pslot = Li[o.node + j] == par ? j : pslot;
      const int q = Li[o.flag + Li[o.tok + i]] - 1;
      if (pslot >= 0 && q >= 0) Li[o.e_fl + K + pslot * NC + q] = 8;
    }
    Li[o.psl + i] = pslot;
  }
  __syncthreads();
  // 3. + 4. the expansion, one thread per entry: (p_nb, p_b), flags (1: a key of the next dp, 2: in `new`), the joint score
  const int ncand = Li[o.misc + TS_NCAND];
  const float pblank = L[o.p + blank];
  const bool blank_in = Li[o.flag + blank] != 0;
  for (int e = tid; e < o.EP; e += nt) {
    if (e >= o.E) {      // padding of the ranking loop: never in front of anything
      L[o.e_sc + e] = NAN;
      continue;
    }
    float nb = -INFINITY, b = -INFINITY, dec = 0.f, lm = 0.f;
    int fl = 0, depth = 0;
    if (e < K) {
      const int node = Li[o.node + e];
      if (node >= 0) {
        const int ci = Li[o.tok + e];
        depth = Li[o.depth + e];
        dec = L[o.dec + e];
        lm = L[o.lm + e];
        if (blank_in) {
          b = pblank + L[o.pl + e];
          fl |= 3;
        }
        if (ci != blank && Li[o.flag + ci] != 0) {
          const float pc = L[o.p + ci];
          nb = pc + L[o.pnb + e];      // the repeated token without a blank between: the prefix stays, and is NOT added to `new`
          fl |= 1;
          const int j = Li[o.psl + e];
          if (j >= 0) {      // the merge: member j extended by ci IS this member
            const float x = ci == Li[o.tok + j] ? pc + L[o.pb + j] : pc + L[o.pl + j];
            nb = ts_lae(nb, x);
            fl |= 3;
          }
        }
      }
    } else {
      const int j = (e - K) / NC, q = (e - K) % NC;
      const int nodej = Li[o.node + j];
      if (nodej >= 0 && q < ncand) {
        const int c = Li[o.cand + q];
        if (c != blank && !(Li[o.e_fl + e] & 8)) {      // (8: this prefix is a beam member, whose own entry takes the contribution)
          const float pc = L[o.p + c];
          nb = c == Li[o.tok + j] ? pc + L[o.pb + j] : pc + L[o.pl + j];
          // expanded in the previous frame and fell off the beam: its mass comes back
          const int key = (nodej + 1) * V + c;
          uint32_t h = ts_hash(key) & (o.HCAP - 1);
          for (int probe = 0; probe < o.HCAP; ++probe) {
            const int kk = Li[o.hkey + h];
            if (kk == key) {
              const float dn = L[o.hnb + h], db = L[o.hb + h];
              b = pblank + ts_lae(dn, db);
              nb = ts_lae(nb, pc + dn);
              break;
            }
            if (kk < 0) break;
            h = (h + 1) & (o.HCAP - 1);
          }
          fl = 3;
          depth = Li[o.depth + j] + 1;
          const int64_t row = ((int64_t)u * K + j) * V + c;
          dec = L[o.dec + j] + (a.dec_rows ? a.dec_rows[row] : 0.f);
          lm = L[o.lm + j] + (a.lm_rows ? a.lm_rows[row] : 0.f);
        }
      }
    }
    float sc = NAN;      // not in `new`: a score no comparison puts in front of another
    if (fl & 2) {
      sc = 0.f;
      if (a.w_ctc != 0.f) sc = a.w_ctc * ts_lae(nb, b);
      if (depth > 0) {
        if (a.dec_rows && a.w_dec != 0.f) sc += a.w_dec * dec;
        if (a.lm_rows && a.w_lm != 0.f) sc += a.w_lm * lm;
      }
      sc += a.pen * (float)depth;
    }
    L[o.e_nb + e] = nb;
    L[o.e_b + e] = b;
    L[o.e_sc + e] = sc;
    L[o.e_dec + e] = dec;
    L[o.e_lm + e] = lm;
    Li[o.e_fl + e] = fl;
  }
  __syncthreads();
  // the previous dp has been read: empty its table
  for (int h = tid; h < o.HCAP; h += nt) Li[o.hkey + h] = -1;
  for (int k = tid; k < K; k += nt) {
    Li[o.sel + k] = -1;
    Li[o.src + k] = -2;
  }
  __syncthreads();
  // 5. the K best of `new`: an entry's rank is the number of entries in front of it (score descending, entry index among equals)
  for (int e = tid; e < o.E; e += nt) {
    if (!(Li[o.e_fl + e] & 2)) continue;
    const float sc = L[o.e_sc + e];
    int rank = 0;
#pragma unroll 8
    for (int e2 = 0; e2 < o.EP; ++e2) {      // (branch-free: the loads of a group are in flight together)
      const float s2 = L[o.e_sc + e2];
      rank += ((s2 > sc) | ((s2 == sc) & (e2 < e))) ? 1 : 0;
    }
    if (rank < K) {
      Li[o.sel + rank] = e;
      Li[o.e_fl + e] |= 4;
    }
  }
  __syncthreads();
  // dp = nxt: every touched prefix that is not in the new beam goes to the table (distinct keys: a claimed place is the key's own)
  for (int e = tid; e < o.E; e += nt) {
    const int fl = Li[o.e_fl + e];
    if (!(fl & 1) || (fl & 4)) continue;
    int key;
    if (e < K) key = (Li[o.par + e] + 1) * V + Li[o.tok + e];
    else key = (Li[o.node + (e - K) / NC] + 1) * V + Li[o.cand + (e - K) % NC];
    uint32_t h = ts_hash(key) & (o.HCAP - 1);
    for (int probe = 0; probe < o.HCAP; ++probe) {
      if (atomicCAS(&Li[o.hkey + h], -1, key) == -1) {
        L[o.hnb + h] = L[o.e_nb + e];
        L[o.hb + h] = L[o.e_b + e];
        break;
      }
      h = (h + 1) & (o.HCAP - 1);
    }
  }
  __syncthreads();
  // the new beam on wave 0, lane = rank: members keep their slot, newcomers take the slots that were given up (ascending, by rank)
  if (tid < 64) {
    const int lane = tid;
    const uint64_t lt = (1ull << lane) - 1ull;
    const int e = lane < K ? Li[o.sel + lane] : -1;
    const bool has = e >= 0, member = has && e < K, newc = has && e >= K;
    bool surv = false;
    if (lane < K)
      for (int r = 0; r < K; ++r) surv = surv || Li[o.sel + r] == lane;
    const uint64_t all = K == 64 ? ~0ull : (1ull << K) - 1ull;
    const uint64_t freem = ~__ballot(surv) & all;
    const int idx = __popcll(__ballot(newc) & lt);
    int slot = member ? e : -1;
    if (newc) {
      uint64_t m = freem;
      for (int q = 0; q < idx; ++q) m &= m - 1;
      slot = __ffsll((unsigned long long)m) - 1;
    }
    float nb = 0.f, b = 0.f, sc = 0.f, dec = 0.f, lm = 0.f;
    int tokv = a.sos, parnode = -1, depth = 0, srcj = -1, node = -1;
    if (has) {
      nb = L[o.e_nb + e]; b = L[o.e_b + e]; sc = L[o.e_sc + e]; dec = L[o.e_dec + e]; lm = L[o.e_lm + e];
      if (member) {
        node = Li[o.node + e]; tokv = Li[o.tok + e]; parnode = Li[o.par + e]; depth = Li[o.depth + e];
      } else {
        srcj = (e - K) / NC;
        tokv = Li[o.cand + (e - K) % NC];
        parnode = Li[o.node + srcj];
        depth = Li[o.depth + srcj] + 1;
      }
    }
    // the newcomer's node: the one its (parent, token) already has in the utterance's table, else a new one
    bool fresh = false;
    int gslot = -1;
    if (newc && slot >= 0) {
      const int key = (parnode + 1) * V + tokv;
      uint32_t h = ts_hash(key) & (o.GCAP - 1);
      for (int probe = 0; probe < o.GCAP; ++probe) {
        const int old = atomicCAS(&wsu[o.gkey + h], -1, key);
        if (old == -1) { fresh = true; gslot = (int)h; break; }
        if (old == key) { node = wsu[o.gval + h]; break; }
        h = (h + 1) & (o.GCAP - 1);
      }
    }
    const uint64_t fm = __ballot(fresh);
    const int nn = Li[o.misc + TS_NNODES];
    if (fresh) {
      node = nn + __popcll(fm & lt);
      if (node < o.NN) {
        wsu[o.gval + gslot] = node;
        wsu[o.tpar + node] = parnode;
        wsu[o.ttok + node] = tokv;
      }
    }
    const bool put = has && slot >= 0 && node >= 0 && node < o.NN;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < K && !surv) Li[o.node + lane] = -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (put) {
      Li[o.node + slot] = node; Li[o.tok + slot] = tokv; Li[o.par + slot] = parnode; Li[o.depth + slot] = depth;
      L[o.pnb + slot] = nb; L[o.pb + slot] = b; L[o.score + slot] = sc; L[o.dec + slot] = dec; L[o.lm + slot] = lm;
      if (newc) Li[o.src + slot] = srcj;
    }
    if (lane < K) Li[o.order + lane] = put ? slot : -1;
    const int nput = __popcll(__ballot(put));
    if (lane == 0) {
      Li[o.misc + TS_NNODES] = nn + __popcll(fm);
      Li[o.misc + TS_NBEAM] = nput;
    }
  }
  __syncthreads();
  // what the scorers need of the slots that are new: token, depth, keys, and the ancestor rows (the parent's list + the own node)
  if (a.tok) {
    const int64_t ld = a.ld_anc;
    for (int k = 0; k < K; ++k) {
      const int src = Li[o.src + k];
      if (src < 0) continue;
      const int64_t n = (int64_t)u * K + k;
      const int depth = Li[o.depth + k];
      if (tid == 0) {
        a.tok[n] = Li[o.tok + k];
        a.pos[n] = depth;
        a.nkeys[n] = depth + 1;
      }
      const int32_t* from = a.anc + ((int64_t)u * K + src) * ld;
      for (int d = tid; d <= depth && d < ld; d += nt)
        a.anc_tmp[n * ld + d] = d < depth ? from[d] : (int32_t)((int64_t)u * o.NN + Li[o.node + k]);
    }
    __syncthreads();      // (a slot that is given up and its parent's list may be one row: staged, then copied)
    for (int k = 0; k < K; ++k) {
      if (Li[o.src + k] < 0) continue;
      const int64_t n = (int64_t)u * K + k;
      const int depth = Li[o.depth + k];
      for (int d = tid; d <= depth && d < ld; d += nt) a.anc[n * ld + d] = a.anc_tmp[n * ld + d];
    }
    __syncthreads();
  }
}

__device__ inline void ts_load(const TsArgs& a, const TsLay& o, float* L, int u) {
  const int32_t* wsu = a.ws + (int64_t)u * o.ws_words;
  int* Li = reinterpret_cast<int*>(L);
  for (int i = threadIdx.x; i < o.persist; i += blockDim.x) Li[i] = wsu[i];
  __syncthreads();
}

__device__ inline void ts_store(const TsArgs& a, const TsLay& o, const float* L, int u) {
  int32_t* wsu = a.ws + (int64_t)u * o.ws_words;
  const int* Li = reinterpret_cast<const int*>(L);
  __syncthreads();
  for (int i = threadIdx.x; i < o.persist; i += blockDim.x) wsu[i] = Li[i];
}

__global__ __launch_bounds__(kTsThreads) void timesync_step_kernel(TsArgs a, TsLay o) {
  extern __shared__ __align__(16) float ts_lds[];
  const int u = blockIdx.x, K = a.K, V = a.V;
  const int t = *a.frame_dev;
  ts_load(a, o, ts_lds, u);
  // the scorer rows of the slots that were new in the previous frame take their places (an utterance past its end still takes them)
  if (a.nkeys) {
    for (int k = 0; k < K; ++k) {
      const int64_t n = (int64_t)u * K + k;
      if (a.nkeys[n] <= 0) continue;
      for (int c = threadIdx.x; c < V; c += blockDim.x) {
        if (a.dec_rows) a.dec_rows[n * V + c] = a.dec_new[n * V + c];
        if (a.lm_rows) a.lm_rows[n * V + c] = a.lm_new[n * V + c];
      }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += blockDim.x) a.nkeys[(int64_t)u * K + k] = 0;
    __syncthreads();
  }
  const int len = (int)min((int64_t)a.T, max((int64_t)0, a.lens[u]));
  if (t >= 0 && t < len) ts_frame(a, o, ts_lds, u, t);
  ts_store(a, o, ts_lds, u);
}

__global__ __launch_bounds__(kTsThreads) void timesync_search_kernel(TsArgs a, TsLay o) {
  extern __shared__ __align__(16) float ts_lds[];
  const int u = blockIdx.x;
  ts_load(a, o, ts_lds, u);
  const int len = (int)min((int64_t)a.T, max((int64_t)0, a.lens[u]));
  for (int t = 0; t < len; ++t) ts_frame(a, o, ts_lds, u, t);
  ts_store(a, o, ts_lds, u);
}

// the state before frame 0: hyps = [(<sos>,)] in slot 0, dp[(<sos>,)] = (-inf, 0), an empty dp table, an empty trie table; slot 0 is
// "new" (the scorers score (<sos>,) once before frame 0), every token operand of the scorers names <sos>
__global__ __launch_bounds__(kTsThreads) void timesync_init_kernel(TsArgs a, TsLay o) {
  const int u = blockIdx.x, K = a.K, tid = threadIdx.x, nt = blockDim.x;
  int32_t* wsu = a.ws + (int64_t)u * o.ws_words;
  float* wf = reinterpret_cast<float*>(wsu);
  for (int i = tid; i < o.persist; i += nt) wsu[i] = 0;
  for (int i = tid; i < o.GCAP; i += nt) { wsu[o.gkey + i] = -1; wsu[o.gval + i] = 0; }
  for (int i = tid; i < o.NN; i += nt) { wsu[o.tpar + i] = -1; wsu[o.ttok + i] = a.sos; }
  __syncthreads();
  for (int i = tid; i < o.HCAP; i += nt) wsu[o.hkey + i] = -1;
  for (int k = tid; k < K; k += nt) {
    wsu[o.node + k] = k == 0 ? 0 : -1;
    wsu[o.tok + k] = a.sos;
    wsu[o.par + k] = -1;
    wf[o.pnb + k] = -INFINITY;
    wf[o.pb + k] = k == 0 ? 0.f : -INFINITY;
    wsu[o.order + k] = k == 0 ? 0 : -1;
    if (a.tok) {
      const int64_t n = (int64_t)u * K + k;
      a.tok[n] = a.sos;
      a.pos[n] = 0;
      a.nkeys[n] = k == 0 ? 1 : 0;
      if (k == 0) a.anc[n * a.ld_anc] = (int32_t)((int64_t)u * o.NN);
    }
  }
  if (tid == 0) {
    wsu[o.misc + TS_NBEAM] = 1;
    wsu[o.misc + TS_NNODES] = 1;
    if (u == 0 && a.frame_dev) *a.frame_dev = 0;
  }
}

// ---------------------------------------------------------------------------------------------- scorer launches, rows at different depths
// tavsr_tree_attn_step with a key count PER ROW: one wave per (row n, head h); a row with 0 keys is skipped (nothing of it is read or
// written).  The row's own key / value (k_new / v_new) is its last key and goes to the pool row its last ancestor entry names.  (Two
// rows of one launch may name one pool row only where a prefix comes back into the beam: both then store the same bits.)
template <int DL>
__global__ __launch_bounds__(256) void tree_attn_rows_kernel(const float* __restrict__ q, int64_t ldq, const float* kpool,
                                                             const float* vpool, int64_t ldkv, const int32_t* __restrict__ anc,
                                                             int64_t ld_anc, const int32_t* __restrict__ nkeys_row, int max_keys,
                                                             float* __restrict__ out, int64_t ldo, int N, int H, int dk, float scale,
                                                             const float* __restrict__ k_new, const float* __restrict__ v_new,
                                                             float* kpool_w, float* vpool_w) {
  constexpr int KG = 64 / DL;
  __shared__ float s_p[4][kTsRowsMaxKeys];
  __shared__ int32_t s_a[4][kTsRowsMaxKeys];
  __shared__ float s_q[4][128];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + wave;
  if (item >= N * H) return;                    // (no workgroup barrier below: a wave is on its own)
  const int n = item / H, h = item % H;
  const int nkeys = min(nkeys_row[n], max_keys);
  if (nkeys <= 0) return;
  const float* qv = q + (int64_t)n * ldq + h * dk;
  const int32_t* a = anc + (int64_t)n * ld_anc;
  for (int d = lane; d < dk; d += 64) s_q[wave][d] = qv[d] * scale;
  for (int j = lane; j < nkeys; j += 64) s_a[wave][j] = a[j];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* klast = k_new + (int64_t)n * ldq + h * dk;
  float mx = -INFINITY;
  for (int j = lane; j < nkeys; j += 64) {
    const float* kr = j == nkeys - 1 ? klast : kpool + (int64_t)s_a[wave][j] * ldkv + h * dk;
    float dot = 0.f;
    for (int d = 0; d < dk; d += 4) {
      const float4 kv = *reinterpret_cast<const float4*>(kr + d);
      dot += s_q[wave][d] * kv.x + s_q[wave][d + 1] * kv.y + s_q[wave][d + 2] * kv.z + s_q[wave][d + 3] * kv.w;
    }
    s_p[wave][j] = dot;
    mx = fmaxf(mx, dot);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < nkeys; j += 64) {
    const float e = expf(s_p[wave][j] - mx);
    s_p[wave][j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float inv = 1.f / sum;
  const int dl = lane & (DL - 1), kg = lane / DL;
  const bool dok = dl * 4 < dk;
  const int doff = h * dk + (dok ? dl * 4 : 0);
  const float* vlast = v_new + (int64_t)n * ldq + doff;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = kg; j < nkeys; j += KG) {
    const float4 v = *reinterpret_cast<const float4*>(j == nkeys - 1 ? vlast : vpool + (int64_t)s_a[wave][j] * ldkv + doff);
    const float pj = s_p[wave][j];
    acc.x += pj * v.x; acc.y += pj * v.y; acc.z += pj * v.z; acc.w += pj * v.w;
  }
#pragma unroll
  for (int o = DL; o < 64; o <<= 1) {
    acc.x += __shfl_xor(acc.x, o, 64); acc.y += __shfl_xor(acc.y, o, 64);
    acc.z += __shfl_xor(acc.z, o, 64); acc.w += __shfl_xor(acc.w, o, 64);
  }
  if (kg == 0 && dok) {
    const int64_t rowp = s_a[wave][nkeys - 1];
    *reinterpret_cast<float4*>(vpool_w + rowp * ldkv + doff) = *reinterpret_cast<const float4*>(vlast);
    *reinterpret_cast<float4*>(kpool_w + rowp * ldkv + doff) = *reinterpret_cast<const float4*>(k_new + (int64_t)n * ldq + doff);
    *reinterpret_cast<float4*>(out + (int64_t)n * ldo + doff) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  }
}

// out[n,:] = table[ids[n],:] * scale + pe[min(max(pos[n], 0), L - 1), :]: tavsr_embed_pe_step with a position per row
__global__ void embed_pe_rows_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table, const float* __restrict__ pe,
                                     float scale, float* __restrict__ out, int64_t total4, int D4, int L,
                                     const int32_t* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total4) return;
  const int64_t n = i / D4;
  const int c4 = (int)(i % D4);
  const int64_t prow = min(max(pos[n], 0), L - 1);
  const float4 e = reinterpret_cast<const float4*>(table)[ids[n] * D4 + c4];
  const float4 p = reinterpret_cast<const float4*>(pe)[prow * D4 + c4];
  reinterpret_cast<float4*>(out)[i] = make_float4(e.x * scale + p.x, e.y * scale + p.y, e.z * scale + p.z, e.w * scale + p.w);
}

static int ts_lds_attr(const void* fn, size_t bytes, const char* what) {
  if (bytes > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kTsLdsBytes);
    TAVSR_REQUIRE(e == hipSuccess, TAVSR_EUNSUPPORTED, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
  }
  return TAVSR_OK;
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_timesync_ok(int32_t K, int32_t V, int32_t T, int32_t C) { return ts_ok(K, V, T, C) ? 1 : 0; }

extern "C" int64_t tavsr_timesync_ws(int32_t K, int32_t V, int32_t T, int32_t C) {
  return ts_ok(K, V, T, C) ? (int64_t)ts_layout(K, V, T, C).ws_words : 0;
}

extern "C" int32_t tavsr_timesync_ws_offset(int32_t K, int32_t V, int32_t T, int32_t C, int32_t which) {
  if (!ts_ok(K, V, T, C)) return -1;
  const TsLay o = ts_layout(K, V, T, C);
  switch (which) {
    case 0: return o.order;
    case 1: return o.node;
    case 2: return o.score;
    case 3: return o.misc;
    case 4: return o.tpar;
    case 5: return o.ttok;
    case 6: return o.NN;
    case 7: return o.NC;
    default: return -1;
  }
}

#define TS_SHAPE_CHECK(name)                                                                                                        \
  TAVSR_REQUIRE(U > 0 && sos >= 0 && sos < V && blank >= 0 && blank < V && sos != blank, TAVSR_EINVAL, name ": bad sizes");          \
  TAVSR_REQUIRE(ts_ok(K, V, T, C), TAVSR_EUNSUPPORTED,                                                                               \
                name ": beam %d, %d tokens, %d frames, pre-beam %d: the frame's tables do not fit one workgroup's LDS (%d bytes), "    \
                "or beam > 64, or pre-beam > tokens, or (3 + beam * frames) * tokens >= 2^31 (tavsr_timesync_ok)", K, V, T, C,          \
                kTsLdsBytes)      /* (the layout is only computed for arguments inside ts_ok's ranges: no size in the message) */

extern "C" int tavsr_timesync_init(int32_t* ws, int64_t* tok, int32_t* pos, int32_t* nkeys, int32_t* anc, int64_t ld_anc,
                                   int32_t* frame_dev, int32_t U, int32_t K, int32_t V, int32_t T, int32_t C, int32_t sos,
                                   int32_t blank, tavsr_stream_t stream) {
  TAVSR_REQUIRE(ws, TAVSR_EINVAL, "timesync_init: null pointer");
  TS_SHAPE_CHECK("timesync_init");
  TAVSR_REQUIRE(!tok || (pos && nkeys && anc && ld_anc >= T + 1), TAVSR_EINVAL,
                "timesync_init: the scorers' operands go together (tok, pos, nkeys, anc with ld_anc >= T + 1)");
  TsArgs a = {};
  a.ws = ws; a.tok = tok; a.pos = pos; a.nkeys = nkeys; a.anc = anc; a.ld_anc = ld_anc; a.frame_dev = frame_dev;
  a.U = U; a.K = K; a.V = V; a.T = T; a.C = C; a.blank = blank; a.sos = sos;
  hipLaunchKernelGGL(timesync_init_kernel, dim3((unsigned)U), dim3(kTsThreads), 0, (hipStream_t)stream, a, ts_layout(K, V, T, C));
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_timesync_step(const float* lpz, const int64_t* lens, int32_t* ws, const float* dec_new, float* dec_rows,
                                   const float* lm_new, float* lm_rows, int64_t* tok, int32_t* pos, int32_t* nkeys, int32_t* anc,
                                   int32_t* anc_tmp, int64_t ld_anc, const int32_t* frame_dev, int32_t U, int32_t K, int32_t V,
                                   int32_t T, int32_t C, int32_t sos, int32_t blank, float w_ctc, float w_dec, float w_lm, float pen,
                                   tavsr_stream_t stream) {
  TAVSR_REQUIRE(lpz && lens && ws && frame_dev, TAVSR_EINVAL, "timesync_step: null pointer");
  TS_SHAPE_CHECK("timesync_step");
  TAVSR_REQUIRE((dec_new == nullptr) == (dec_rows == nullptr) && (lm_new == nullptr) == (lm_rows == nullptr), TAVSR_EINVAL,
                "timesync_step: a scorer's new rows and its kept rows go together");
  TAVSR_REQUIRE(tok ? (pos && nkeys && anc && anc_tmp && ld_anc >= T + 1) : (!dec_rows && !lm_rows), TAVSR_EINVAL,
                "timesync_step: scorer rows need the scorers' operands (tok, pos, nkeys, anc, anc_tmp with ld_anc >= T + 1)");
  const TsLay o = ts_layout(K, V, T, C);
  const size_t bytes = (size_t)o.lds_words * 4;
  if (int rc = ts_lds_attr(reinterpret_cast<const void*>(timesync_step_kernel), bytes, "timesync_step")) return rc;
  TsArgs a = {};
  a.lpz = lpz; a.lens = lens; a.ws = ws; a.dec_new = dec_new; a.dec_rows = dec_rows; a.lm_new = lm_new; a.lm_rows = lm_rows;
  a.tok = tok; a.pos = pos; a.nkeys = nkeys; a.anc = anc; a.anc_tmp = anc_tmp; a.ld_anc = ld_anc;
  a.frame_dev = const_cast<int32_t*>(frame_dev);
  a.U = U; a.K = K; a.V = V; a.T = T; a.C = C; a.blank = blank; a.sos = sos;
  a.w_ctc = w_ctc; a.w_dec = w_dec; a.w_lm = w_lm; a.pen = pen;
  hipLaunchKernelGGL(timesync_step_kernel, dim3((unsigned)U), dim3(kTsThreads), bytes, (hipStream_t)stream, a, o);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_timesync_search(const float* lpz, const int64_t* lens, int32_t* ws, int32_t U, int32_t K, int32_t V, int32_t T,
                                     int32_t C, int32_t sos, int32_t blank, float w_ctc, float pen, tavsr_stream_t stream) {
  TAVSR_REQUIRE(lpz && lens && ws, TAVSR_EINVAL, "timesync_search: null pointer");
  TS_SHAPE_CHECK("timesync_search");
  const TsLay o = ts_layout(K, V, T, C);
  const size_t bytes = (size_t)o.lds_words * 4;
  if (int rc = ts_lds_attr(reinterpret_cast<const void*>(timesync_search_kernel), bytes, "timesync_search")) return rc;
  TsArgs a = {};
  a.lpz = lpz; a.lens = lens; a.ws = ws;
  a.U = U; a.K = K; a.V = V; a.T = T; a.C = C; a.blank = blank; a.sos = sos;
  a.w_ctc = w_ctc; a.pen = pen;
  hipLaunchKernelGGL(timesync_search_kernel, dim3((unsigned)U), dim3(kTsThreads), bytes, (hipStream_t)stream, a, o);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_tree_attn_rows(const float* q, int64_t ldq, const float* kpool, const float* vpool, int64_t ldkv,
                                    const int32_t* anc, int64_t ld_anc, const int32_t* nkeys_row, int32_t max_keys, float* out,
                                    int64_t ldo, int32_t N, int32_t H, int32_t dk, float scale, const float* k_new,
                                    const float* v_new, tavsr_stream_t stream) {
  TAVSR_REQUIRE(q && kpool && vpool && anc && nkeys_row && out && k_new && v_new, TAVSR_EINVAL, "tree_attn_rows: null pointer");
  TAVSR_REQUIRE(max_keys > 0 && max_keys <= kTsRowsMaxKeys && max_keys <= ld_anc, TAVSR_EUNSUPPORTED,
                "tree_attn_rows: 1..%d keys per row within the ancestor lists (got %d)", kTsRowsMaxKeys, max_keys);
  TAVSR_REQUIRE(dk % 4 == 0 && dk <= 128 && ldkv % 4 == 0 && ldq % 4 == 0 && ldo % 4 == 0 &&
                    (((uintptr_t)q | (uintptr_t)out | (uintptr_t)kpool | (uintptr_t)vpool | (uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0,
                TAVSR_EALIGN, "tree_attn_rows: dk %% 4, dk <= 128 and 16-byte aligned rows are required");
  if (N <= 0) return TAVSR_OK;
  const dim3 grid((unsigned)((N * H + 3) / 4)), block(256);
  if (dk <= 64)
    hipLaunchKernelGGL(tree_attn_rows_kernel<16>, grid, block, 0, (hipStream_t)stream, q, ldq, kpool, vpool, ldkv, anc, ld_anc,
                       nkeys_row, max_keys, out, ldo, N, H, dk, scale, k_new, v_new, const_cast<float*>(kpool),
                       const_cast<float*>(vpool));
  else
    hipLaunchKernelGGL(tree_attn_rows_kernel<32>, grid, block, 0, (hipStream_t)stream, q, ldq, kpool, vpool, ldkv, anc, ld_anc,
                       nkeys_row, max_keys, out, ldo, N, H, dk, scale, k_new, v_new, const_cast<float*>(kpool),
                       const_cast<float*>(vpool));
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_embed_pe_rows(const int64_t* ids, const float* table, const float* pe, float scale, float* out, int64_t N,
                                   int32_t L, int32_t D, const int32_t* pos, tavsr_stream_t stream) {
  TAVSR_REQUIRE(ids && table && pe && out && pos, TAVSR_EINVAL, "embed_pe_rows: null pointer");
  TAVSR_REQUIRE(D % 4 == 0 && L > 0, TAVSR_EINVAL, "embed_pe_rows: D %% 4 == 0 required");
  if (N <= 0) return TAVSR_OK;
  const int64_t total4 = N * (D / 4);
  hipLaunchKernelGGL(embed_pe_rows_kernel, dim3(cdiv(total4, 256)), dim3(256), 0, (hipStream_t)stream, ids, table, pe, scale, out,
                     total4, D / 4, L, pos);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
