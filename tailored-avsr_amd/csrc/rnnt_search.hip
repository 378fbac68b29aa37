// Transducer beam searches: alignment-length synchronous decoding (ALSD) and time-synchronous decoding (TSD) of espnet2
// asr/transducer/beam_search_transducer.py for a ragged batch, K = beam rows per utterance.  Contracts: include/tavsr.h.
// One step of a search is a chain of launches (tavsr/inference/transducer.py replays it as a graph): the joint rows at a frame
// per row, a log-softmax / top-K reduce per row, the per-utterance bookkeeping (one workgroup per utterance, its candidate
// tables in LDS), and the gather of the prediction network's states by parent slot in front of tavsr_lstm_step.  The state
// that lives across launches (the beam, the trie of prefixes with its open-addressing table, ALSD's `final` list, TSD's A
// list) is the utterance's block of the int32 workspace; nothing here reads a value on the host and no sum uses an atomic.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

namespace tavsr {

constexpr int kSearchMaxK = 64;
constexpr int kSearchMaxExp = 8;
constexpr int kSearchThreads = 256;
constexpr int kSearchLdsBytes = 160 * 1024;
enum { kAlsd = 0, kTsd = 1 };
// header words of an utterance's block
enum { kHStep = 0, kHSlots = 1, kHNodes = 2, kHList = 3, kHOverflow = 4, kHdrWords = 16 };

// word offsets inside an utterance's block.  node / score / len [K]: the beam (ALSD's B, TSD's C and, between frames, B; len:
// ALSD's label count per member, TSD does not keep it); parent / token [nodes]: the trie, node 0 = (blank,); hp / ht / hv
// [tab]: its table keyed by (parent node, token), hv = node or -1; lnode / lscore [list]: ALSD's final, TSD's A.
struct SearchLayout {
  int32_t node, score, len, parent, token, hp, ht, hv, lnode, lscore, words;
  int32_t nodes, tab, list;
};

static int64_t r64(int64_t n) { return (n + 63) / 64 * 64; }

static bool search_layout(int kind, int64_t K, int64_t T, int64_t u_max, int64_t M, SearchLayout* out) {
  if ((kind != kAlsd && kind != kTsd) || K < 1 || K > kSearchMaxK || T < 1 || u_max < 0 || M < 1 || M > kSearchMaxExp) return false;
  const int64_t um = u_max < T - 1 ? u_max : T - 1;
  const int64_t nodes = kind == kAlsd ? 1 + K * (T + um) : 1 + K * T * (M - 1);
  const int64_t list = kind == kAlsd ? K * (T + um) : K * M;
  int64_t tab = 64;
  while (tab < 2 * nodes) tab *= 2;
  int64_t o = kHdrWords;
  SearchLayout l;
  auto take = [&](int64_t n) { const int64_t at = o; o += r64(n); return (int32_t)at; };
  if (3 * r64(K) + 2 * r64(nodes) + 3 * tab + 2 * r64(list) + kHdrWords >= ((int64_t)1 << 30)) return false;
  l.node = take(K); l.score = take(K); l.len = take(K);
  l.parent = take(nodes); l.token = take(nodes);
  l.hp = take(tab); l.ht = take(tab); l.hv = take(tab);
  l.lnode = take(list); l.lscore = take(list);
  l.words = (int32_t)o;
  l.nodes = (int32_t)nodes; l.tab = (int32_t)tab; l.list = (int32_t)list;
  if (out) *out = l;
  return true;
}

// LDS of a step's workgroup, in 4-byte words: the candidate scores (ALSD: A = K (K + 1); TSD: max(D = K K, A = K M)), the
// selection [K], the beam as it was (node, len, score, frame: 4 K), the beam as it will be (node, score, len, parent, token: 5 K)
// and one word per member for ALSD's "is in B_" flags
static int64_t search_lds_words(int kind, int64_t K, int64_t M) {
  const int64_t cand = kind == kAlsd ? K * (K + 1) : (K * K > K * M ? K * K : K * M);
  return cand + 11 * K;
}

static bool search_ok(int kind, int64_t K, int64_t V, int64_t T, int64_t u_max, int64_t M) {
  return search_layout(kind, K, T, u_max, M, nullptr) && V > K && search_lds_words(kind, K, M) * 4 <= kSearchLdsBytes;
}

__device__ __forceinline__ int clamp_len(const int64_t* tlens, int u, int T) {
  const int64_t t = tlens[u];
  return (int)(t < 0 ? 0 : (t < T ? t : T));
}

__device__ __forceinline__ float log_add(float a, float b) {
  if (a == -INFINITY) return b;
  if (b == -INFINITY) return a;
  const float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}

// the node of (parent, token): found, or made.  One thread per utterance calls this, in a fixed order.
__device__ int trie_node(int32_t* blk, const SearchLayout& L, int parent, int token) {
  uint32_t h = (uint32_t)parent * 2654435761u ^ (uint32_t)token * 0x85ebca6bu;
  h ^= h >> 15;
  const uint32_t mask = (uint32_t)L.tab - 1;
  h &= mask;
  for (int probe = 0; probe < L.tab; ++probe) {
    const int v = blk[L.hv + h];
    if (v < 0) {
      const int n = blk[kHNodes];
      if (n >= L.nodes) { blk[kHOverflow] = 1; return parent; }
      blk[L.parent + n] = parent;
      blk[L.token + n] = token;
      blk[L.hp + h] = parent; blk[L.ht + h] = token; blk[L.hv + h] = n;
      blk[kHNodes] = n + 1;
      return n;
    }
    if (blk[L.hp + h] == parent && blk[L.ht + h] == token) return v;
    h = (h + 1) & mask;
  }
  blk[kHOverflow] = 1;
  return parent;
}

__global__ __launch_bounds__(kSearchThreads) void rnnt_search_init_kernel(int32_t* __restrict__ ws, const SearchLayout L,
                                                                          const int64_t* __restrict__ tlens,
                                                                          int32_t* __restrict__ row_t, int K, int T) {
  const int u = blockIdx.x, tid = threadIdx.x;
  int32_t* blk = ws + (int64_t)u * L.words;
  for (int i = tid; i < kHdrWords; i += kSearchThreads) blk[i] = i == kHSlots || i == kHNodes ? 1 : 0;
  for (int k = tid; k < K; k += kSearchThreads) {
    blk[L.node + k] = k == 0 ? 0 : -1;
    blk[L.score + k] = __float_as_int(0.f);
    blk[L.len + k] = 0;
    row_t[u * K + k] = k == 0 && clamp_len(tlens, u, T) > 0 ? 0 : -1;
  }
  for (int i = tid; i < L.tab; i += kSearchThreads) blk[L.hv + i] = -1;
  if (tid == 0) { blk[L.parent] = -1; blk[L.token] = 0; }
}

// z[n][:] = tanh(e[n / K][row_t[n]][:] + d[n][:]); a skipped row (row_t < 0) is 0 and reads no frame
__global__ void rnnt_search_z_kernel(const float* __restrict__ e, const float* __restrict__ d, const int32_t* __restrict__ row_t,
                                     float* __restrict__ z, int N, int K, int T, int J) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)N * J) return;
  const int n = (int)(i / J), c = (int)(i - (int64_t)n * J);
  const int t = min(row_t[n], T - 1);
  z[i] = t >= 0 ? tanh_fast(e[((int64_t)(n / K) * T + t) * J + c] + d[i]) : 0.f;
}

// One workgroup per row: log-softmax, lp_blank = logp[0], and the K best labels (ids >= 1) in descending order, the lower id
// first among equal values.  Pick k is the greatest element behind pick k - 1 in that order, so nothing is marked or moved.
__global__ __launch_bounds__(kSearchThreads) void rnnt_row_topk_kernel(const float* __restrict__ logits, int64_t ldv,
                                                                       const int32_t* __restrict__ row_t, float* __restrict__ lp_blank,
                                                                       float* __restrict__ topv, int32_t* __restrict__ topi, int V, int K) {
  __shared__ float s_f[2][kSearchThreads / 64];
  __shared__ int s_i[2][kSearchThreads / 64];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (row_t && row_t[row] < 0) return;
  const float* x = logits + (int64_t)row * ldv;
  float mx = -FLT_MAX;
  for (int v = tid; v < V; v += kSearchThreads) mx = fmaxf(mx, x[v]);
  mx = wave_max(mx);
  if (lane == 0) s_f[0][wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_f[0][0], s_f[0][1]), fmaxf(s_f[0][2], s_f[0][3]));
  float se = 0.f;
  for (int v = tid; v < V; v += kSearchThreads) se += expf(x[v] - mx);
  se = wave_sum(se);
  if (lane == 0) s_f[1][wv] = se;
  __syncthreads();
  const float lse = mx + logf(((s_f[1][0] + s_f[1][1]) + s_f[1][2]) + s_f[1][3]);
  if (tid == 0) lp_blank[row] = x[0] - lse;
  float lastv = INFINITY;
  int lasti = -1;
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY;
    int bi = INT_MAX;
    for (int v = 1 + tid; v < V; v += kSearchThreads) {
      const float xv = x[v];
      const bool behind = xv < lastv || (xv == lastv && v > lasti);
      if (behind && (xv > best || (xv == best && v < bi))) { best = xv; bi = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { s_f[k & 1][wv] = best; s_i[k & 1][wv] = bi; }      // (parity k & 1 was last read before pick k - 1's barrier)
    __syncthreads();
    best = s_f[k & 1][0]; bi = s_i[k & 1][0];
#pragma unroll
    for (int w = 1; w < kSearchThreads / 64; ++w) {
      const float ob = s_f[k & 1][w];
      const int oi = s_i[k & 1][w];
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    lastv = best; lasti = bi;
    if (tid == 0) {
      topv[(int64_t)row * K + k] = best - lse;
      topi[(int64_t)row * K + k] = bi < V ? bi : V - 1;      // (bi stays INT_MAX only where fewer than K labels compare: NaN rows)
    }
  }
}

// dst[l][n][:] = src[l][idx[n]][:] for both state tensors; idx[n] < 0 leaves row n alone
__global__ void rnnt_gather_state_kernel(const float* __restrict__ sh, const float* __restrict__ sc, const int32_t* __restrict__ idx,
                                         float* __restrict__ dh, float* __restrict__ dc, int L, int Ns, int Nd, int H) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)L * Nd * H) return;
  const int c = (int)(i % H);
  const int64_t ln = i / H;
  const int n = (int)(ln % Nd), l = (int)(ln / Nd);
  const int s = idx[n];
  if (s < 0 || s >= Ns) return;
  const int64_t from = ((int64_t)l * Ns + s) * H + c;
  dh[i] = sh[from];
  dc[i] = sc[from];
}

// rank of candidate j among the valid ones in descending order, earlier index first among equals (a stable sort's place)
__device__ __forceinline__ int stable_rank(const float* cand, const uint8_t* valid_of, int n, int group, int j) {
  const float s = cand[j];
  int rank = 0, j2 = 0;
  for (int k2 = 0; j2 < n; ++k2) {
    const bool ok = valid_of == nullptr || valid_of[k2];
    for (int m2 = 0; m2 < group && j2 < n; ++m2, ++j2) {
      const float s2 = cand[j2];
      rank += (ok && (s2 > s || (s2 == s && j2 < j))) ? 1 : 0;
    }
  }
  return rank;
}

struct StepLds {
  float* cand;
  int *sel, *o_node, *o_len, *o_t, *n_node, *n_len, *n_par, *n_tok;
  float *o_score, *n_score;
  __device__ StepLds(float* sm, int ncand, int K) {
    cand = sm;
    sel = reinterpret_cast<int*>(sm + ncand);
    o_node = sel + K; o_len = o_node + K; o_t = o_len + K;
    o_score = reinterpret_cast<float*>(o_t + K);
    n_node = reinterpret_cast<int*>(o_score + K); n_len = n_node + K; n_par = n_len + K; n_tok = n_par + K;
    n_score = reinterpret_cast<float*>(n_tok + K);
  }
};

// an utterance with nothing to do in this launch: the state update that follows copies every row onto itself
__device__ __forceinline__ void rows_keep(int u, int K, int32_t* parent, int64_t* tok, uint8_t* commit) {
  for (int k = threadIdx.x; k < K; k += kSearchThreads) {
    parent[u * K + k] = u * K + k;
    tok[u * K + k] = 0;
    commit[u * K + k] = 0;
  }
}

// One value of i of align_length_sync_decoding for utterance blockIdx.x.
__global__ __launch_bounds__(kSearchThreads) void rnnt_alsd_step_kernel(int32_t* __restrict__ ws, const SearchLayout L,
                                                                        const int64_t* __restrict__ tlens, const float* __restrict__ lpb,
                                                                        const float* __restrict__ topv, const int32_t* __restrict__ topi,
                                                                        int32_t* __restrict__ row_t, int32_t* __restrict__ parent,
                                                                        int64_t* __restrict__ tok, uint8_t* __restrict__ commit, int K,
                                                                        int T, int u_max) {
  extern __shared__ float sm[];
  const int G = K + 1, n = K * G;
  StepLds s(sm, n, K);
  uint8_t* s_act = reinterpret_cast<uint8_t*>(s.n_score + K);      // [K]: the member is in B_
  const int u = blockIdx.x, tid = threadIdx.x;
  int32_t* blk = ws + (int64_t)u * L.words;
  const int Tu = clamp_len(tlens, u, T);
  const int steps = Tu > 0 ? Tu + min(u_max, Tu - 1) : 0;
  const int i = blk[kHStep], nb = blk[kHSlots];
  if (i >= steps) {
    rows_keep(u, K, parent, tok, commit);
    for (int k = tid; k < K; k += kSearchThreads) row_t[u * K + k] = -1;
    return;
  }
  for (int k = tid; k < K; k += kSearchThreads) {
    s.o_node[k] = blk[L.node + k];
    s.o_len[k] = blk[L.len + k];
    s.o_score[k] = __int_as_float(blk[L.score + k]);
    s.o_t[k] = k < nb ? row_t[u * K + k] : -1;
    s_act[k] = s.o_t[k] >= 0;
    s.sel[k] = 0;
  }
  __syncthreads();
  int nact = 0;
  for (int k = 0; k < K; ++k) nact += s_act[k];
  for (int j = tid; j < n; j += kSearchThreads) {
    const int k = j / G, m = j - k * G;
    float v = -INFINITY;
    if (s_act[k]) {
      const int64_t r = (int64_t)u * K + k;
      v = s.o_score[k] + (m == 0 ? lpb[r] : topv[r * K + m - 1]);
    }
    s.cand[j] = v;
  }
  __syncthreads();
  if (nact == 0) {      // B_ is empty: B stays as it is
    rows_keep(u, K, parent, tok, commit);
    for (int k = tid; k < K; k += kSearchThreads) row_t[u * K + k] = -1;
    if (tid == 0) blk[kHStep] = i + 1;
    return;
  }
  const int nsel = min(K, nact * G);
  for (int j = tid; j < n; j += kSearchThreads) {
    if (!s_act[j / G]) continue;
    const int rank = stable_rank(s.cand, s_act, n, G, j);
    if (rank < K) s.sel[rank] = j;
  }
  __syncthreads();
  if (tid == 0) {
    int nf = blk[kHList];
    for (int k = 0; k < nb; ++k) {      // the blank extensions at the last frame, in B_'s order
      if (s.o_t[k] != Tu - 1) continue;
      if (nf >= L.list) { blk[kHOverflow] = 1; break; }
      blk[L.lnode + nf] = s.o_node[k];
      blk[L.lscore + nf] = __float_as_int(s.cand[k * G]);
      ++nf;
    }
    blk[kHList] = nf;
    int nnew = 0;
    for (int r = 0; r < nsel; ++r) {      // the beam best, recombined: the first of equal prefixes keeps its place
      const int j = s.sel[r], k = j / G, m = j - k * G;
      const float sc = s.cand[j];
      int node = s.o_node[k], len = s.o_len[k], tk = -1;
      if (m > 0) {
        tk = topi[((int64_t)u * K + k) * K + m - 1];
        node = trie_node(blk, L, node, tk);
        ++len;
      }
      int at = -1;
      for (int q = 0; q < nnew && at < 0; ++q)
        if (s.n_node[q] == node) at = q;
      if (at >= 0) {
        s.n_score[at] = log_add(s.n_score[at], sc);
      } else {
        s.n_node[nnew] = node; s.n_score[nnew] = sc; s.n_len[nnew] = len; s.n_par[nnew] = k; s.n_tok[nnew] = tk;
        ++nnew;
      }
    }
    blk[kHSlots] = nnew;
    blk[kHStep] = i + 1;
    s.sel[0] = nnew;
  }
  __syncthreads();
  const int nnew = s.sel[0];
  for (int k = tid; k < K; k += kSearchThreads) {
    const int r = u * K + k;
    const bool in = k < nnew;
    blk[L.node + k] = in ? s.n_node[k] : -1;
    blk[L.score + k] = __float_as_int(in ? s.n_score[k] : 0.f);
    blk[L.len + k] = in ? s.n_len[k] : 0;
    const bool label = in && s.n_tok[k] >= 0;
    parent[r] = u * K + (in ? s.n_par[k] : k);
    tok[r] = label ? s.n_tok[k] : 0;
    commit[r] = label ? 1 : 0;
    const int t = i + 1 - (in ? s.n_len[k] : 0);
    row_t[r] = in && i + 1 < steps && t <= Tu - 1 ? t : -1;
  }
}

// Expansion v of one frame of time_sync_decoding for utterance blockIdx.x.  The rows of the beam are C; A is the block's list.
//   every v: a member of C whose prefix A held before this v adds its blank extension into that entry; any other is appended,
//            and a_src[u K M + place] names its row (-1 elsewhere): the launch behind this one copies the row's state there.
//   v < M-1: C = the K best label extensions of C (parent / tok / commit = 1 per new row: gather, then one LSTM step).
//   v = M-1: B = the K best of A; b_sel[row] names the A place whose state the row takes (-1: none); the frame advances.
__global__ __launch_bounds__(kSearchThreads) void rnnt_tsd_step_kernel(int32_t* __restrict__ ws, const SearchLayout L,
                                                                       const int64_t* __restrict__ tlens, const float* __restrict__ lpb,
                                                                       const float* __restrict__ topv, const int32_t* __restrict__ topi,
                                                                       int32_t* __restrict__ row_t, int32_t* __restrict__ parent,
                                                                       int64_t* __restrict__ tok, uint8_t* __restrict__ commit,
                                                                       int32_t* __restrict__ a_src, int32_t* __restrict__ b_sel, int v, int K,
                                                                       int T, int M) {
  extern __shared__ float sm[];
  const int KM = K * M, ncand = max(K * K, KM);
  StepLds s(sm, ncand, K);
  const int u = blockIdx.x, tid = threadIdx.x;
  const bool last = v == M - 1;
  int32_t* blk = ws + (int64_t)u * L.words;
  const int Tu = clamp_len(tlens, u, T);
  const int t = blk[kHStep], nc = blk[kHSlots];
  for (int p = tid; p < KM; p += kSearchThreads) a_src[u * KM + p] = -1;
  for (int k = tid; k < K; k += kSearchThreads) b_sel[u * K + k] = -1;
  if (t >= Tu) {
    rows_keep(u, K, parent, tok, commit);
    for (int k = tid; k < K; k += kSearchThreads) row_t[u * K + k] = -1;
    return;
  }
  for (int k = tid; k < K; k += kSearchThreads) {
    s.o_node[k] = blk[L.node + k];
    s.o_score[k] = __int_as_float(blk[L.score + k]);
    s.sel[k] = 0;
  }
  __syncthreads();      // (also orders the a_src fill in front of thread 0's entries)
  if (tid == 0) {
    const int seen = v == 0 ? 0 : blk[kHList];
    int na = seen;
    for (int k = 0; k < nc; ++k) {
      const float sb = s.o_score[k] + lpb[u * K + k];
      int at = -1;
      for (int q = 0; q < seen && at < 0; ++q)
        if (blk[L.lnode + q] == s.o_node[k]) at = q;
      if (at >= 0) {
        blk[L.lscore + at] = __float_as_int(log_add(__int_as_float(blk[L.lscore + at]), sb));
      } else if (na < L.list) {
        blk[L.lnode + na] = s.o_node[k];
        blk[L.lscore + na] = __float_as_int(sb);
        a_src[u * KM + na] = u * K + k;
        ++na;
      } else {
        blk[kHOverflow] = 1;
      }
    }
    blk[kHList] = na;
    s.sel[0] = na;
  }
  __syncthreads();
  const int na = s.sel[0];
  __syncthreads();
  if (!last) {
    const int n = nc * K, nsel = min(K, n);
    for (int j = tid; j < n; j += kSearchThreads) {
      const int k = j / K;
      s.cand[j] = s.o_score[k] + topv[((int64_t)u * K + k) * K + (j - k * K)];
    }
    __syncthreads();
    for (int j = tid; j < n; j += kSearchThreads) {
      const int rank = stable_rank(s.cand, nullptr, n, K, j);
      if (rank < K) s.sel[rank] = j;
    }
    __syncthreads();
    if (tid == 0) {
      for (int r = 0; r < nsel; ++r) {
        const int j = s.sel[r], k = j / K;
        const int tk = topi[((int64_t)u * K + k) * K + (j - k * K)];
        s.n_node[r] = trie_node(blk, L, s.o_node[k], tk);
        s.n_score[r] = s.cand[j]; s.n_par[r] = k; s.n_tok[r] = tk;
      }
      blk[kHSlots] = nsel;
    }
    __syncthreads();
    for (int k = tid; k < K; k += kSearchThreads) {
      const int r = u * K + k;
      const bool in = k < nsel;
      blk[L.node + k] = in ? s.n_node[k] : -1;
      blk[L.score + k] = __float_as_int(in ? s.n_score[k] : 0.f);
      parent[r] = u * K + (in ? s.n_par[k] : k);
      tok[r] = in ? s.n_tok[k] : 0;
      commit[r] = in ? 1 : 0;
      row_t[r] = in ? t : -1;
    }
  } else {
    const int nsel = min(K, na);
    for (int j = tid; j < na; j += kSearchThreads) s.cand[j] = __int_as_float(blk[L.lscore + j]);
    __syncthreads();
    for (int j = tid; j < na; j += kSearchThreads) {
      const int rank = stable_rank(s.cand, nullptr, na, na, j);
      if (rank < K) s.sel[rank] = j;
    }
    __syncthreads();
    rows_keep(u, K, parent, tok, commit);
    for (int k = tid; k < K; k += kSearchThreads) {
      const int r = u * K + k;
      const bool in = k < nsel;
      const int j = in ? s.sel[k] : 0;
      blk[L.node + k] = in ? blk[L.lnode + j] : -1;
      blk[L.score + k] = __float_as_int(in ? s.cand[j] : 0.f);
      b_sel[r] = in ? u * KM + j : -1;
      row_t[r] = in && t + 1 < Tu ? t + 1 : -1;
    }
    if (tid == 0) { blk[kHSlots] = nsel; blk[kHStep] = t + 1; }
  }
}

}  // namespace tavsr

using namespace tavsr;

extern "C" int tavsr_rnnt_search_ok(int32_t kind, int32_t K, int32_t V, int32_t T, int32_t u_max, int32_t max_sym_exp) {
  return search_ok(kind, K, V, T, u_max, max_sym_exp) ? 1 : 0;
}

extern "C" int64_t tavsr_rnnt_search_ws(int32_t kind, int32_t K, int32_t T, int32_t u_max, int32_t max_sym_exp) {
  SearchLayout l;
  return search_layout(kind, K, T, u_max, max_sym_exp, &l) ? l.words : 0;
}

extern "C" int32_t tavsr_rnnt_search_ws_offset(int32_t kind, int32_t K, int32_t T, int32_t u_max, int32_t max_sym_exp, int32_t which) {
  SearchLayout l;
  if (!search_layout(kind, K, T, u_max, max_sym_exp, &l)) return -1;
  const int32_t off[] = {l.node, l.score, l.len, l.parent, l.token, l.lnode, l.lscore, l.nodes, l.list};
  return which >= 0 && which < (int32_t)(sizeof off / sizeof off[0]) ? off[which] : -1;
}

#define SEARCH_SHAPE_OR_RETURN(what, kind, K, V, T, u_max, M, l)                                                                   \
  TAVSR_REQUIRE(search_ok(kind, K, V, T, u_max, M) && search_layout(kind, K, T, u_max, M, &l), TAVSR_EUNSUPPORTED,                 \
                what ": beam %d, %d tokens, %d frames, u_max %d, max_sym_exp %d is not supported (tavsr_rnnt_search_ok): 1 <= "   \
                "beam <= %d, beam < tokens, 1 <= max_sym_exp <= %d, the trie within 2^30 words",                                  \
                (int)(K), (int)(V), (int)(T), (int)(u_max), (int)(M), kSearchMaxK, kSearchMaxExp)

extern "C" int tavsr_rnnt_search_init(int32_t* ws, const int64_t* tlens, int32_t* row_t, int32_t U, int32_t kind, int32_t K, int32_t V,
                                      int32_t T, int32_t u_max, int32_t max_sym_exp, tavsr_stream_t stream) {
  SearchLayout l;
  SEARCH_SHAPE_OR_RETURN("rnnt_search_init", kind, K, V, T, u_max, max_sym_exp, l);
  if (U <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(ws && tlens && row_t, TAVSR_EINVAL, "rnnt_search_init: null pointer");
  TAVSR_REQUIRE((int64_t)U * K < ((int64_t)1 << 24), TAVSR_EUNSUPPORTED, "rnnt_search_init: %d utterances x beam %d rows", U, K);
  hipLaunchKernelGGL(rnnt_search_init_kernel, dim3(U), dim3(kSearchThreads), 0, (hipStream_t)stream, ws, l, tlens, row_t, K, T);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_search_z(const float* e, const float* d, const int32_t* row_t, float* z, int32_t N, int32_t K, int32_t T,
                                   int32_t J, tavsr_stream_t stream) {
  if (N <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(e && d && row_t && z && K > 0 && T > 0 && J > 0 && N % K == 0, TAVSR_EINVAL, "rnnt_search_z: null pointer or bad sizes");
  hipLaunchKernelGGL(rnnt_search_z_kernel, dim3(cdiv((int64_t)N * J, 256)), dim3(256), 0, (hipStream_t)stream, e, d, row_t, z, N, K, T, J);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_row_topk(const float* logits, int64_t ldv, const int32_t* row_t, float* lp_blank, float* topv, int32_t* topi,
                                   int32_t N, int32_t V, int32_t K, tavsr_stream_t stream) {
  if (N <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(logits && lp_blank && topv && topi, TAVSR_EINVAL, "rnnt_row_topk: null pointer");
  TAVSR_REQUIRE(K >= 1 && K <= kSearchMaxK && V > K && ldv >= V, TAVSR_EUNSUPPORTED,
                "rnnt_row_topk: 1 <= K <= %d and K < V <= ldv (K=%d V=%d ldv=%lld)", kSearchMaxK, K, V, (long long)ldv);
  hipLaunchKernelGGL(rnnt_row_topk_kernel, dim3(N), dim3(kSearchThreads), 0, (hipStream_t)stream, logits, ldv, row_t, lp_blank, topv, topi,
                     V, K);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_gather_state(const float* src_h, const float* src_c, const int32_t* idx, float* dst_h, float* dst_c, int32_t L,
                                       int32_t Ns, int32_t Nd, int32_t H, tavsr_stream_t stream) {
  if (L <= 0 || Nd <= 0 || H <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(src_h && src_c && idx && dst_h && dst_c && Ns > 0, TAVSR_EINVAL, "rnnt_gather_state: null pointer or no source rows");
  TAVSR_REQUIRE(src_h != dst_h && src_c != dst_c, TAVSR_EINVAL, "rnnt_gather_state: the gather is not done in place");
  hipLaunchKernelGGL(rnnt_gather_state_kernel, dim3(cdiv((int64_t)L * Nd * H, 256)), dim3(256), 0, (hipStream_t)stream, src_h, src_c, idx,
                     dst_h, dst_c, L, Ns, Nd, H);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_alsd_step(int32_t* ws, const int64_t* tlens, const float* lp_blank, const float* topv, const int32_t* topi,
                                    int32_t* row_t, int32_t* parent, int64_t* tok, uint8_t* commit, int32_t U, int32_t K, int32_t V,
                                    int32_t T, int32_t u_max, tavsr_stream_t stream) {
  SearchLayout l;
  SEARCH_SHAPE_OR_RETURN("rnnt_alsd_step", kAlsd, K, V, T, u_max, 1, l);
  if (U <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(ws && tlens && lp_blank && topv && topi && row_t && parent && tok && commit, TAVSR_EINVAL, "rnnt_alsd_step: null pointer");
  const size_t lds = (size_t)search_lds_words(kAlsd, K, 1) * 4;
  hipLaunchKernelGGL(rnnt_alsd_step_kernel, dim3(U), dim3(kSearchThreads), lds, (hipStream_t)stream, ws, l, tlens, lp_blank, topv, topi, row_t,
                     parent, tok, commit, K, T, u_max);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}

extern "C" int tavsr_rnnt_tsd_step(int32_t* ws, const int64_t* tlens, const float* lp_blank, const float* topv, const int32_t* topi,
                                   int32_t* row_t, int32_t* parent, int64_t* tok, uint8_t* commit, int32_t* a_src, int32_t* b_sel,
                                   int32_t v, int32_t U, int32_t K, int32_t V, int32_t T, int32_t max_sym_exp, tavsr_stream_t stream) {
  SearchLayout l;
  SEARCH_SHAPE_OR_RETURN("rnnt_tsd_step", kTsd, K, V, T, 0, max_sym_exp, l);
  if (U <= 0) return TAVSR_OK;
  TAVSR_REQUIRE(ws && tlens && lp_blank && topv && topi && row_t && parent && tok && commit && a_src && b_sel, TAVSR_EINVAL,
                "rnnt_tsd_step: null pointer");
  TAVSR_REQUIRE(v >= 0 && v < max_sym_exp, TAVSR_EINVAL, "rnnt_tsd_step: expansion %d of %d", v, max_sym_exp);
  const size_t lds = (size_t)search_lds_words(kTsd, K, max_sym_exp) * 4;
  hipLaunchKernelGGL(rnnt_tsd_step_kernel, dim3(U), dim3(kSearchThreads), lds, (hipStream_t)stream, ws, l, tlens, lp_blank, topv, topi, row_t,
                     parent, tok, commit, a_src, b_sel, v, K, T, max_sym_exp);
  TAVSR_LAUNCH_CHECK();
  return TAVSR_OK;
}
