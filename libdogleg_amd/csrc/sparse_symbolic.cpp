// sparse_symbolic.cpp -- see sparse_symbolic.h.  Pure host code (no HIP).  The front of the symbolic phase, one function
// per step, two of the four threaded schedules (9a, 10) and sym_analyze, which calls them in order; the interfaces
// between them are in sparse_symbolic_internal.h.
#include "sparse_symbolic_internal.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>
#include <cmath>
#include <numeric>
#include <queue>

int env_int(const char* name, int dflt)
{
  const char* s = getenv(name);
  return (s && *s) ? atoi(s) : dflt;
}

SymKnobs sym_knobs_env()
{
  SymKnobs K;
  K.slice_cap = env_int("DOGLEG_AMD_SLICE_CAP", SYM_FAC_LDS_BUDGET/8 - 40);
  K.nd_leaf = env_int("DOGLEG_AMD_ND_LEAF", 300);
  K.lds_split = env_int("DOGLEG_AMD_LDS_SPLIT", 1) != 0;
  K.mf_level = env_int("DOGLEG_AMD_MF_LEVEL", 1);
  K.syrk_min = env_int("DOGLEG_AMD_SYRK_MIN", 100);
  K.asm_mfma = env_int("DOGLEG_AMD_ASM_MFMA", 1);
  K.rider_min = env_int("DOGLEG_AMD_RIDER_MIN", 4096);
  K.debug = env_int("DOGLEG_AMD_SYM_DEBUG", 0);
  return K;
}

namespace {

constexpr int VB_MAX   = 8;       // max variables per var-block (<= 64 lanes per 8x8 output block)
constexpr int RB_MAX   = 8;       // max rows per row-block
constexpr int CH_JTX   = 128;     // contributions per Jt*x wave-task (long lists are latency chains: keep them short)
constexpr int MAXCH_JTX = 2048;
constexpr int PANEL_CAP = 16384;  // doubles: supernode panels up to this size are factored in LDS
constexpr int SN_WMAX  = 256;     // max supernode width

// ---------------------------------------------------- nested dissection -----
struct Orderer
{
  const Graph& G;
  std::vector<char> removed;      // dense nodes and already-ordered separators
  std::vector<int>  mark;         // generic stamp array
  int stamp = 0;
  std::vector<int>  out;          // resulting order (node ids)
  int leaf_w;

  Orderer(const Graph& g, int leaf_w_) : G(g), removed(g.n, 0), mark(g.n, 0), leaf_w(leaf_w_) {}

  // BFS over `in_set`-stamped nodes from root; fills levels; returns eccentricity
  int bfs(int root, int setstamp, std::vector<int>& order, std::vector<int>& lvl_start,
          std::vector<int>& dist)
  {
    order.clear(); lvl_start.clear();
    ++stamp;
    const int visited = stamp;
    order.push_back(root); vis[root] = visited; dist[root] = 0;
    lvl_start.push_back(0);
    size_t head = 0;
    int cur = 0;
    while(head < order.size())
    {
      const int u = order[head];
      if(dist[u] != cur) { cur = dist[u]; lvl_start.push_back((int)head); }
      head++;
      for(int e = G.ptr[u]; e < G.ptr[u+1]; e++)
      {
        const int v = G.adj[e];
        if(inset[v] != setstamp || vis[v] == visited) continue;
        vis[v] = visited; dist[v] = dist[u] + 1; order.push_back(v);
      }
    }
    lvl_start.push_back((int)order.size());
    return cur;
  }
  std::vector<int> inset, vis;

  // exact minimum degree on a small induced subgraph (leaf of the dissection)
  void order_leaf(const std::vector<int>& nodes)
  {
    const int n = (int)nodes.size();
    if(n > 4000)
    {
      std::vector<int> s(nodes);
      std::sort(s.begin(), s.end(), [&](int a, int b) {
        if(G.wdeg[a] != G.wdeg[b]) return G.wdeg[a] < G.wdeg[b];
        return a < b; });
      out.insert(out.end(), s.begin(), s.end());
      return;
    }
    // local ids
    ++stamp;
    std::vector<int> lid_of;           // via mark: store local id in a side map
    static thread_local std::vector<int> loc;
    if((int)loc.size() < G.n) loc.assign(G.n, -1);
    for(int i = 0; i < n; i++) loc[nodes[i]] = i;
    std::vector<std::vector<int>> adj(n);
    std::vector<long> ext(n, 0);       // weight of neighbours outside the leaf (static)
    for(int i = 0; i < n; i++)
    {
      const int u = nodes[i];
      for(int e = G.ptr[u]; e < G.ptr[u+1]; e++)
      {
        const int v = G.adj[e];
        if(loc[v] >= 0 && inset[v] == inset[u] && loc[v] < n && nodes[loc[v]] == v) adj[i].push_back(loc[v]);
        else ext[i] += G.w[v];
      }
      std::sort(adj[i].begin(), adj[i].end());
    }
    std::vector<char> gone(n, 0);
    std::vector<long> deg(n);
    auto wdeg = [&](int i) { long d = ext[i]; for(int v : adj[i]) d += G.w[nodes[v]]; return d; };
    for(int i = 0; i < n; i++) deg[i] = wdeg(i);
    std::vector<int> tmp;
    for(int it = 0; it < n; it++)
    {
      int best = -1;
      for(int i = 0; i < n; i++)
        if(!gone[i] && (best < 0 || deg[i] < deg[best] || (deg[i] == deg[best] && nodes[i] < nodes[best]))) best = i;
      gone[best] = 1;
      out.push_back(nodes[best]);
      // neighbours of best become a clique
      const std::vector<int>& nb = adj[best];
      for(int v : nb)
      {
        tmp.clear();
        std::set_union(adj[v].begin(), adj[v].end(), nb.begin(), nb.end(), std::back_inserter(tmp));
        // drop v itself and best
        std::vector<int> nv; nv.reserve(tmp.size());
        for(int x : tmp) if(x != v && x != best) nv.push_back(x);
        adj[v].swap(nv);
      }
      // the eliminated node's external weight is inherited by its neighbours' fill only
      for(int v : nb) deg[v] = wdeg(v);
      adj[best].clear();
    }
    for(int i = 0; i < n; i++) loc[nodes[i]] = -1;
  }

  void run(const std::vector<int>& all_nodes)
  {
    inset.assign(G.n, 0); vis.assign(G.n, 0);
    std::vector<int> dist(G.n, 0);
    int setctr = 0;
    // explicit stack of node sets; a frame with `sep` set flushes a separator
    struct Frame { std::vector<int> nodes; bool is_sep; };
    std::vector<Frame> stack;
    stack.push_back({all_nodes, false});
    std::vector<int> order, lvl_start, comp;
    while(!stack.empty())
    {
      Frame f = std::move(stack.back());
      stack.pop_back();
      if(f.is_sep) { out.insert(out.end(), f.nodes.begin(), f.nodes.end()); continue; }
      if(f.nodes.empty()) continue;
      // stamp the set
      const int setstamp = ++setctr;
      for(int u : f.nodes) inset[u] = setstamp;
      // split into connected components; process each
      std::vector<std::vector<int>> comps;
      ++stamp;
      const int cstamp = stamp;
      for(int u : f.nodes)
      {
        if(vis[u] == cstamp) continue;
        comp.clear(); comp.push_back(u); vis[u] = cstamp;
        for(size_t h = 0; h < comp.size(); h++)
        {
          const int a = comp[h];
          for(int e = G.ptr[a]; e < G.ptr[a+1]; e++)
          {
            const int v = G.adj[e];
            if(inset[v] == setstamp && vis[v] != cstamp) { vis[v] = cstamp; comp.push_back(v); }
          }
        }
        comps.push_back(comp);
      }
      if(comps.size() > 1)
      {
        // push in reverse so that the first component is ordered first
        for(size_t c = comps.size(); c-- > 0;) stack.push_back({std::move(comps[c]), false});
        continue;
      }
      std::vector<int>& nodes = comps[0];
      long wt = 0; for(int u : nodes) wt += G.w[u];
      if(wt <= leaf_w || nodes.size() <= 3) { std::sort(nodes.begin(), nodes.end()); order_leaf(nodes); continue; }
      // pseudo-peripheral root: a few BFS sweeps from the min-degree node
      int root = nodes[0];
      for(int u : nodes) if(G.wdeg[u] < G.wdeg[root] || (G.wdeg[u] == G.wdeg[root] && u < root)) root = u;
      int ecc = bfs(root, setstamp, order, lvl_start, dist);
      for(int sweep = 0; sweep < 3; sweep++)
      {
        // candidate: min-degree node of the last level
        const int nl = (int)lvl_start.size() - 1;
        int cand = order[lvl_start[nl-1]];
        for(int i = lvl_start[nl-1]; i < lvl_start[nl]; i++)
          if(G.wdeg[order[i]] < G.wdeg[cand]) cand = order[i];
        std::vector<int> o2, l2;
        const int e2 = bfs(cand, setstamp, o2, l2, dist);
        if(e2 > ecc) { ecc = e2; root = cand; order.swap(o2); lvl_start.swap(l2); }
        else { bfs(root, setstamp, order, lvl_start, dist); break; }
      }
      const int nl = (int)lvl_start.size() - 1;
      if(nl < 3) { std::sort(nodes.begin(), nodes.end()); order_leaf(nodes); continue; }
      // level weights, choose the lightest level whose prefix weight is within [0.3,0.7]
      std::vector<long> lw(nl, 0);
      for(int l = 0; l < nl; l++) for(int i = lvl_start[l]; i < lvl_start[l+1]; i++) lw[l] += G.w[order[i]];
      long pre = 0; int best = -1; double bestscore = 0;
      for(int l = 0; l < nl; l++)
      {
        const double before = (double)pre/(double)wt, after = (double)(wt - pre - lw[l])/(double)wt;
        pre += lw[l];
        if(l == 0 || l == nl-1) continue;
        if(before < 0.25 || after < 0.25) continue;
        // score: small separators first, balance as tie-break
        const double score = (double)lw[l]*(1.0 + 0.5*fabs(before - after));
        if(best < 0 || score < bestscore) { best = l; bestscore = score; }
      }
      if(best < 0)
      {
        // no balanced level: take the middle one by weight
        pre = 0;
        for(int l = 0; l < nl; l++) { pre += lw[l]; if(2*pre >= wt) { best = l; break; } }
        if(best <= 0) best = 1;
        if(best >= nl-1) best = nl-2;
      }
      std::vector<int> A(order.begin(), order.begin() + lvl_start[best]);
      std::vector<int> Sp(order.begin() + lvl_start[best], order.begin() + lvl_start[best+1]);
      std::vector<int> B(order.begin() + lvl_start[best+1], order.end());
      if(A.empty() || B.empty()) { std::sort(nodes.begin(), nodes.end()); order_leaf(nodes); continue; }
      std::sort(Sp.begin(), Sp.end());
      // order: A ..., B ..., then the separator (stack is LIFO)
      stack.push_back({std::move(Sp), true});
      stack.push_back({std::move(B), false});
      stack.push_back({std::move(A), false});
    }
  }
};

// the block-level elimination tree: parent and number of children of every block position, scalar weight of its structure
struct BlockTree { std::vector<int> parent, nchild; std::vector<long> stw; };

// ---------------------------------------------------------- 1. var-blocks
int sym_var_blocks(int N, int M, const int* cp, const int* ri, SymHost& S, SymFront& F, std::vector<int>& vb_of, char* err, int errlen)
{
  std::vector<char> cut(N + 1, 0);
  cut[0] = cut[N] = 1;
  for(int r = 0; r < M; r++)
  {
    const int a = cp[r], b = cp[r+1];
    if(b < a) SYM_FAIL("Jt column pointers must be non-decreasing (row %d)", r);
    if(b - a > 65535) SYM_FAIL("measurement row %d has %d non-zeros; at most 65535 are supported", r, b - a);
    for(int q = a; q < b; q++)
    {
      const int i = ri[q];
      if(i < 0 || i >= N) SYM_FAIL("row index %d out of range in measurement %d", i, r);
      if(q > a && ri[q-1] >= i) SYM_FAIL("row indices of measurement %d are not strictly ascending", r);
      if(q == a   || ri[q-1] != i-1) cut[i] = 1;
      if(q == b-1 || ri[q+1] != i+1) cut[i+1] = 1;
    }
  }
  vb_of.resize(N);
  {
    int start = 0;
    for(int j = 1; j <= N; j++)
      if(cut[j] || j - start == VB_MAX) { cut[j] = 1; start = j; }
    S.vb_start.clear();
    for(int j = 0; j <= N; j++) if(cut[j]) S.vb_start.push_back(j);
    S.nvb = (int)S.vb_start.size() - 1;
    for(int v = 0; v < S.nvb; v++) for(int j = S.vb_start[v]; j < S.vb_start[v+1]; j++) vb_of[j] = v;
  }
  F.N = N; F.nvb = S.nvb;
  F.w.resize(S.nvb);
  for(int v = 0; v < S.nvb; v++) F.w[v] = S.vb_start[v+1] - S.vb_start[v];
  return 0;
}

// ---------------------------------------------------------- 2. row-blocks
void sym_row_blocks(int M, const int* cp, const int* ri, int row0, int row1, const std::vector<int>& vb_of, const SymHost& S, SymFront& F)
{
  int cur = -1;
  for(int r = 0; r < M; r++)
  {
    const int len = cp[r+1] - cp[r];
    if(len == 0) { cur = -1; continue; }
    bool fresh = (cur < 0) || r == row0 || r == row1;
    if(!fresh)
    {
      const RowBlock& b = F.rbs[cur];
      if(b.len != len || b.nrows == RB_MAX || b.r0 + b.nrows != r ||
         memcmp(&ri[b.base], &ri[cp[r]], sizeof(int)*(size_t)len) != 0) fresh = true;
    }
    if(fresh)
    {
      RowBlock b; b.r0 = r; b.nrows = 1; b.len = len; b.base = cp[r]; b.vptr = (int)F.rb_vb.size();
      b.local = (r >= row0 && r < row1);
      b.lbase = b.base - cp[row0]; b.lr0 = r - row0;
      int e = 0;
      while(e < len)
      {
        const int v = vb_of[ri[b.base + e]];
        F.rb_vb.push_back(v); F.rb_off.push_back(e);
        e += S.vb_start[v+1] - ri[b.base + e];     // remainder of the block from this entry
      }
      b.nvb = (int)F.rb_vb.size() - b.vptr;
      F.rbs.push_back(b);
      cur = (int)F.rbs.size() - 1;
    }
    else F.rbs[cur].nrows++;
  }
  F.nrb = (int)F.rbs.size();
}

// ------------------------------------------------ 3. block graph of JtJ
void sym_block_graph(const SymFront& F, Graph& G, int64_t& nnz_JtJ_lower)
{
  const int nvb = F.nvb, nrb = F.nrb;
  G.n = nvb; G.w = F.w;
  {
    // inverted index vb -> row-blocks; skip row-blocks with a pattern identical to the previous one
    std::vector<int> cnt(nvb + 1, 0);
    std::vector<char> dup(nrb, 0);
    for(int b = 1; b < nrb; b++)
      if(F.rbs[b].nvb == F.rbs[b-1].nvb &&
         memcmp(&F.rb_vb[F.rbs[b].vptr], &F.rb_vb[F.rbs[b-1].vptr], sizeof(int)*(size_t)F.rbs[b].nvb) == 0) dup[b] = 1;
    for(int b = 0; b < nrb; b++) if(!dup[b]) for(int k = 0; k < F.rbs[b].nvb; k++) cnt[F.rb_vb[F.rbs[b].vptr + k] + 1]++;
    for(int v = 0; v < nvb; v++) cnt[v+1] += cnt[v];
    std::vector<int> inv(cnt[nvb]), nxt(cnt.begin(), cnt.end() - 1);
    for(int b = 0; b < nrb; b++) if(!dup[b]) for(int k = 0; k < F.rbs[b].nvb; k++) inv[nxt[F.rb_vb[F.rbs[b].vptr + k]]++] = b;
    std::vector<int> mark(nvb, -1);
    G.ptr.assign(nvb + 1, 0);
    std::vector<int> tmp;
    for(int v = 0; v < nvb; v++)
    {
      tmp.clear();
      mark[v] = v;
      for(int a = cnt[v]; a < cnt[v+1]; a++)
      {
        const RowBlock& b = F.rbs[inv[a]];
        for(int k = 0; k < b.nvb; k++)
        {
          const int u = F.rb_vb[b.vptr + k];
          if(mark[u] != v) { mark[u] = v; tmp.push_back(u); }
        }
      }
      std::sort(tmp.begin(), tmp.end());
      G.adj.insert(G.adj.end(), tmp.begin(), tmp.end());
      G.ptr[v+1] = (int)G.adj.size();
    }
    G.wdeg.assign(nvb, 0);
    for(int v = 0; v < nvb; v++) for(int e = G.ptr[v]; e < G.ptr[v+1]; e++) G.wdeg[v] += G.w[G.adj[e]];
  }
  // nnz(tril JtJ)
  nnz_JtJ_lower = 0;
  for(int v = 0; v < nvb; v++)
  {
    const long w = G.w[v];
    nnz_JtJ_lower += w*(w+1)/2;
    for(int e = G.ptr[v]; e < G.ptr[v+1]; e++) if(G.adj[e] > v) nnz_JtJ_lower += w*G.w[G.adj[e]];
  }
}

// ------------------------------------------------------------ 4. ordering
int sym_ordering(const Graph& G, const SymKnobs& K, SymFront& F, char* err, int errlen)
{
  const int N = F.N, nvb = F.nvb;
  F.border.clear();            // position -> vb
  {
    const double dense_thr = std::max(16.0, 10.0*sqrt((double)N));
    std::vector<int> sparse_nodes, dense_nodes;
    Graph H;                           // graph without dense nodes
    std::vector<char> is_dense(nvb, 0);
    for(int v = 0; v < nvb; v++) if((double)G.wdeg[v] > dense_thr && nvb > 8) is_dense[v] = 1;
    for(int v = 0; v < nvb; v++) (is_dense[v] ? dense_nodes : sparse_nodes).push_back(v);
    H.n = nvb; H.w = G.w; H.ptr.assign(nvb + 1, 0);
    for(int v = 0; v < nvb; v++)
    {
      if(!is_dense[v]) for(int e = G.ptr[v]; e < G.ptr[v+1]; e++) if(!is_dense[G.adj[e]]) H.adj.push_back(G.adj[e]);
      H.ptr[v+1] = (int)H.adj.size();
    }
    H.wdeg = G.wdeg;
    Orderer O(H, K.nd_leaf);
    O.run(sparse_nodes);
    F.border = O.out;
    // dense nodes last, lightest first
    std::sort(dense_nodes.begin(), dense_nodes.end(), [&](int a, int b) {
      if(G.wdeg[a] != G.wdeg[b]) return G.wdeg[a] < G.wdeg[b];
      return a < b; });
    F.border.insert(F.border.end(), dense_nodes.begin(), dense_nodes.end());
    if((int)F.border.size() != nvb) SYM_FAIL("internal error: ordering lost blocks (%zu of %d)", F.border.size(), nvb);
  }
  F.bpos.resize(nvb);
  for(int k = 0; k < nvb; k++) F.bpos[F.border[k]] = k;
  return 0;
}

// the structure of every block column and the elimination tree under the order F.border
void block_symbolic(const Graph& G, SymFront& F, BlockTree& T)
{
  const int nvb = F.nvb;
  std::vector<int> head(nvb, -1), next(nvb, -1), mark(nvb, -1);
  std::vector<int> tmp;
  std::fill(T.parent.begin(), T.parent.end(), -1);
  std::fill(T.nchild.begin(), T.nchild.end(), 0);
  for(int j = 0; j < nvb; j++)
  {
    tmp.clear();
    mark[j] = j;
    const int v = F.border[j];
    for(int e = G.ptr[v]; e < G.ptr[v+1]; e++)
    {
      const int q = F.bpos[G.adj[e]];
      if(q > j && mark[q] != j) { mark[q] = j; tmp.push_back(q); }
    }
    for(int c = head[j]; c >= 0; c = next[c])
    {
      for(int q : F.st[c]) if(q > j && mark[q] != j) { mark[q] = j; tmp.push_back(q); }
    }
    std::sort(tmp.begin(), tmp.end());
    F.st[j] = tmp;
    if(!tmp.empty()) { T.parent[j] = tmp[0]; next[j] = head[tmp[0]]; head[tmp[0]] = j; T.nchild[tmp[0]]++; }
  }
}

// --------------------------------- 5. block-level symbolic factorisation
int sym_block_factor(const Graph& G, SymFront& F, BlockTree& T, SymHost& S, char* err, int errlen)
{
  const int nvb = F.nvb;
  F.st.assign(nvb, {});        // struct of block column (positions > j), sorted
  T.parent.assign(nvb, -1); T.nchild.assign(nvb, 0);
  block_symbolic(G, F, T);
  // Leaves of the elimination tree with IDENTICAL structure (e.g. the points seen by
  // the same set of cameras) are independent of each other; placed next to each other
  // they form one supernode with a block-diagonal top -> far fewer, wider panels
  // (rank-k updates instead of k rank-3 ones).  Moving a leaf earlier is always a
  // valid elimination order.
  {
    std::vector<int> leaves;
    for(int j = 0; j < nvb; j++) if(T.nchild[j] == 0 && !F.st[j].empty()) leaves.push_back(j);
    std::sort(leaves.begin(), leaves.end(), [&](int x, int y) {
      if(F.st[x] != F.st[y]) return F.st[x] < F.st[y];
      return x < y; });
    std::vector<int> group_of(nvb, -1), group_first;
    std::vector<std::vector<int>> members;
    for(size_t i = 0; i < leaves.size();)
    {
      size_t k = i + 1;
      while(k < leaves.size() && F.st[leaves[k]] == F.st[leaves[i]]) k++;
      if(k - i > 1)
      {
        std::vector<int> m(leaves.begin() + i, leaves.begin() + k);      // ascending positions
        for(int x : m) group_of[x] = (int)members.size();
        members.push_back(m);
      }
      i = k;
    }
    // New order: every leaf first (grouped by structure, groups and single leaves by
    // first position), then the remaining nodes in a POSTORDER of the elimination tree
    // restricted to them.  With the leaves out of the way a chain of the tree (e.g. the
    // cameras of one dissection leaf, whose other children are all points) becomes a run
    // of consecutive columns and merges into one supernode.
    {
      std::vector<char> is_leaf(nvb, 0);
      for(int j : leaves) is_leaf[j] = 1;
      std::vector<int> nb; nb.reserve(nvb);
      std::vector<char> done(members.size(), 0);
      for(int j = 0; j < nvb; j++)
      {
        if(!is_leaf[j]) continue;
        const int g = group_of[j];
        if(g < 0) { nb.push_back(F.border[j]); continue; }
        if(done[g]) continue;
        done[g] = 1;
        for(int x : members[g]) nb.push_back(F.border[x]);
      }
      // children lists of the non-leaf forest
      std::vector<int> chead(nvb, -1), cnext(nvb, -1);
      std::vector<int> roots;
      for(int j = nvb - 1; j >= 0; j--)
      {
        if(is_leaf[j]) continue;
        if(T.parent[j] >= 0) { cnext[j] = chead[T.parent[j]]; chead[T.parent[j]] = j; }   // ascending child lists
        else roots.push_back(j);
      }
      std::sort(roots.begin(), roots.end());
      std::vector<int> stack, it(nvb, -2);
      for(int r : roots)
      {
        stack.push_back(r);
        while(!stack.empty())
        {
          const int u = stack.back();
          if(it[u] == -2) it[u] = chead[u];
          if(it[u] >= 0) { const int c = it[u]; it[u] = cnext[c]; stack.push_back(c); }
          else { nb.push_back(F.border[u]); stack.pop_back(); }
        }
      }
      if((int)nb.size() != nvb) SYM_FAIL("internal error: postorder lost blocks (%zu of %d)", nb.size(), nvb);
      F.border.swap(nb);
      for(int k = 0; k < nvb; k++) F.bpos[F.border[k]] = k;
      block_symbolic(G, F, T);
    }
  }
  T.stw.assign(nvb, 0);                   // scalar weight of struct
  for(int j = 0; j < nvb; j++) for(int q : F.st[j]) T.stw[j] += G.w[F.border[q]];
  S.nnz_L = 0; S.factor_flops = 0;
  for(int j = 0; j < nvb; j++)
  {
    const long w = G.w[F.border[j]];
    S.nnz_L += w*(w+1)/2 + w*T.stw[j];
    for(long a = 0; a < w; a++) { const double c = (double)(w - a + T.stw[j]); S.factor_flops += c*c; }
  }
  return 0;
}

// ------------------------------------------------------- 6. supernodes
void sym_supernodes(const BlockTree& T, const SymKnobs& K, SymFront& F, std::vector<char>& sn_bd)
{
  const int nvb = F.nvb;
  F.sn_b0.clear();             // first block position of each supernode (+ sentinel)
  sn_bd.clear();               // supernode made of sibling leaves only: block-diagonal top
  {
    const int relax = 25;
    const int sib_w = 64;
    const int split_w = 32;   // columns from which a run stays a supernode of its own beside its T.parent's other children
    const long chain_cap = PANEL_CAP;   // width cap of chain supernodes: W*(W+64)
    const bool lds_split = K.lds_split;
    const long lds_split_minw = 32;
    // width of the fundamental supernode (maximal chain of exactly nested block columns) starting at j:
    // a relaxed merge across a structure change takes that whole run or nothing -- stopping in the
    // middle of it at the width cap leaves fragments that cost an elimination-tree level each
    std::vector<long> run_w(nvb + 1, 0);
    for(int j = nvb - 1; j >= 0; j--)
    {
      const bool exact_next = j + 1 < nvb && T.parent[j] == j + 1 && F.st[j].size() == F.st[j+1].size() + 1;
      run_w[j] = F.w[F.border[j]] + (exact_next ? run_w[j+1] : 0);
    }
    // children lists and the longest chain of columns below (and including) every block column
    std::vector<int> kid_head(nvb, -1), kid_next(nvb, -1);
    std::vector<long> crit(nvb, 0);
    for(int j = 0; j < nvb; j++)
    {
      crit[j] += F.w[F.border[j]];
      if(T.parent[j] >= 0)
      {
        kid_next[j] = kid_head[T.parent[j]]; kid_head[T.parent[j]] = j;
        crit[T.parent[j]] = std::max(crit[T.parent[j]], crit[j]);
      }
    }
    int a = 0;
    long W = F.w[F.border[0]];              // current width
    long true_nnz = W*T.stw[0];             // sum_j w_j * |struct_j| (scalar) for columns in the supernode
    long below_own = 0;                   // helper: sum_j w_j * (own cols after j)
    F.sn_b0.push_back(0);
    bool sib_only = true; int nmerge = 0;
    for(int j = 0; j + 1 <= nvb; j++)
    {
      bool merge = false;
      if(j + 1 < nvb && T.parent[j] == j + 1)
      {
        const long w1 = F.w[F.border[j+1]];
        const long Wn = W + w1, Rn = T.stw[j+1];
        // zeros in the rectangular-below + trapezoid-own storage if merged
        const long tn = true_nnz + w1*T.stw[j+1];
        // stored (excluding the dense diagonal block): every column holds Rn below rows + own cols after it
        long own_after = below_own + W*w1;    // each existing column gains w1 own rows after it
        const long stored = Wn*Rn + own_after;
        const long zeros = stored - tn;
        const bool exact = (F.st[j].size() == F.st[j+1].size() + 1);
        // a panel is factored in row slices (>= 64 rows each) that all carry the w x w top block
        // (... unless it has fewer rows below than that: the root of the tree, whose panel is its top block)
        const long below = std::min<long>(64, Rn);
        const bool fits = (Wn*(Wn + below) <= chain_cap) && Wn <= SN_WMAX;
        const long Wrun = W + run_w[j+1];
        const bool run_fits = (Wrun*(Wrun + below) <= chain_cap) && Wrun <= SN_WMAX;
        // A wide run of columns is NOT merged into a T.parent that has other children: merged, it is eliminated
        // after all of them (the merged supernode waits for every child); on its own it is eliminated beside
        // them.  The top of a nested dissection: the separator of one half and the root separator -- 60
        // columns less on the critical path of config #4.
        // Costs in columns on the critical path (crit[c]: the longest chain of columns ending with block c):
        // merged, the supernode starts when ALL children are done -- max(crit[j], sib + W) to its end --, apart
        // the run ends at crit[j] and the T.parent starts at max(crit[j], sib) plus one more hand-off (~split_w
        // columns' worth).  Siblings that are leaves (points) never make it worth it.
        long sib = 0;
        if(T.nchild[j+1] >= 2)
          for(int c = kid_head[j+1]; c >= 0; c = kid_next[c]) if(c != j) sib = std::max(sib, crit[c]);
        const bool beside_siblings = T.nchild[j+1] >= 2 && std::min<long>(W, sib + W - crit[j]) > split_w;
        // A chain whose panel would not fit LDS whole is cut where it still does, once it is wide enough to be worth a
        // workgroup (config #5: separators of 96 columns with 194 rows below, 222 KB -- as one supernode they are cut into
        // ROW slices, which keeps every level above the leaves out of the multifrontal one-launch region; as 64 + 32
        // columns both panels fit and the whole top of the tree is one launch).
        const long pan_n = ((Wn + Rn + 1 + 1) & ~1L)*Wn;
        const bool lds_cut = lds_split && W >= lds_split_minw && pan_n > K.slice_cap && Rn + 1 <= 255;
        if(fits && !beside_siblings && !lds_cut && (exact || (run_fits && (Wn <= 16 || zeros*100 <= (long)relax*(stored + Wn*Wn)))))
        {
          merge = true; sib_only = false; nmerge++;
          W = Wn; true_nnz = tn; below_own = own_after;
        }
      }
      if(!merge && j + 1 < nvb && T.nchild[j] == 0 && T.nchild[j+1] == 0 && !F.st[j].empty() && F.st[j] == F.st[j+1])
      {
        // sibling leaves with identical structure: block-diagonal top, same rows below
        const long w1 = F.w[F.border[j+1]];
        const long Wn = W + w1, Rn = T.stw[j+1];
        if(Wn <= sib_w && (Wn + Rn + 1)*Wn <= PANEL_CAP)
        {
          merge = true; nmerge++;
          true_nnz += w1*T.stw[j+1]; below_own += W*w1; W = Wn;
        }
      }
      if(!merge && j + 1 < nvb)
      {
        sn_bd.push_back((sib_only && nmerge > 0) ? 1 : 0); sib_only = true; nmerge = 0;
        a = j + 1; F.sn_b0.push_back(a);
        W = F.w[F.border[a]]; true_nnz = W*T.stw[a]; below_own = 0;
      }
    }
    sn_bd.push_back((sib_only && nmerge > 0) ? 1 : 0);
    F.sn_b0.push_back(nvb);
  }
  F.nsn = (int)F.sn_b0.size() - 1;
}

// ------------------------------------------- 7. scalar-level layout
void sym_layout(const BlockTree& T, const std::vector<char>& sn_bd, SymFront& F, SymHost& S)
{
  const int N = F.N, nvb = F.nvb, nsn = F.nsn;
  S.nsn = nsn;
  F.colstart.assign(nvb + 1, 0);  // scalar position of block position
  for(int k = 0; k < nvb; k++) F.colstart[k+1] = F.colstart[k] + F.w[F.border[k]];
  S.perm.resize(N); S.iperm.resize(N);
  for(int k = 0; k < nvb; k++)
    for(int a = 0; a < F.w[F.border[k]]; a++)
    { S.perm[F.colstart[k] + a] = S.vb_start[F.border[k]] + a; S.iperm[S.vb_start[F.border[k]] + a] = F.colstart[k] + a; }
  F.sn_of_b.resize(nvb);
  S.sn_c0.resize(nsn + 1); S.sn_rowptr.assign(nsn + 1, 0); S.sn_lx.assign(nsn + 1, 0); S.sn_scr.assign(nsn + 1, 0);
  // block-level below structure of a supernode = struct of its last block column
  auto sn_last = [&](int s) { return F.sn_b0[s+1] - 1; };
  for(int s = 0; s < nsn; s++)
  {
    for(int k = F.sn_b0[s]; k < F.sn_b0[s+1]; k++) F.sn_of_b[k] = s;
    S.sn_c0[s] = F.colstart[F.sn_b0[s]];
  }
  S.sn_c0[nsn] = N;
  // members (var-blocks) of the block-diagonal supernodes
  S.sn_bd_ptr.assign(nsn + 1, 0);
  for(int s2 = 0; s2 < nsn; s2++)
  {
    if(sn_bd[s2]) for(int k = F.sn_b0[s2]; k < F.sn_b0[s2+1]; k++) S.sn_bd_col.push_back(F.colstart[k] - F.colstart[F.sn_b0[s2]]);
    S.sn_bd_ptr[s2+1] = (int)S.sn_bd_col.size();
  }
  S.max_panel = 0;
  for(int s = 0; s < nsn; s++)
  {
    const int w = S.sn_c0[s+1] - S.sn_c0[s];
    const long r = T.stw[sn_last(s)];
    const long nrows = w + r + 1;          // + the augmented right-hand-side row (see sparse_symbolic.h)
    S.sn_rowptr[s+1] = S.sn_rowptr[s] + (int)nrows;
    S.sn_lx[s+1] = S.sn_lx[s] + nrows*(long)w;
    S.sn_scr[s+1] = S.sn_scr[s] + (int)r;
    if(nrows*w > S.max_panel) S.max_panel = (int)(nrows*w);
  }
  S.lx_size = S.sn_lx[nsn]; S.scr_size = S.sn_scr[nsn];
  S.sn_rows.resize(S.sn_rowptr[nsn]);
  // per supernode: block-level row offsets of the below blocks (for lookups)
  F.belowoff_ptr.assign(nsn + 1, 0);
  for(int s = 0; s < nsn; s++) F.belowoff_ptr[s+1] = F.belowoff_ptr[s] + (int)F.below(s).size();
  F.belowoff.resize(F.belowoff_ptr[nsn]);
  for(int s = 0; s < nsn; s++)
  {
    int* rows = &S.sn_rows[S.sn_rowptr[s]];
    const int w = S.sn_c0[s+1] - S.sn_c0[s];
    int k = 0;
    for(; k < w; k++) rows[k] = S.sn_c0[s] + k;
    int bi = F.belowoff_ptr[s];
    for(int q : F.below(s))
    {
      F.belowoff[bi++] = k;
      for(int a = 0; a < F.w[F.border[q]]; a++) rows[k++] = F.colstart[q] + a;
    }
    rows[k++] = N;                         // augmented row: virtual variable N, present in every panel
  }
  S.diagpos.resize(N); S.col_sn.resize(N);
  for(int s = 0; s < nsn; s++)
  {
    const int w = S.sn_c0[s+1] - S.sn_c0[s];
    const long ld = S.sn_rowptr[s+1] - S.sn_rowptr[s];
    for(int c = 0; c < w; c++) { S.diagpos[S.sn_c0[s] + c] = S.sn_lx[s] + c + c*ld; S.col_sn[S.sn_c0[s] + c] = s; }
  }

  // levels
  S.sn_level.assign(nsn, 0);
  for(int s = 0; s < nsn; s++)
  {
    const std::vector<int>& bl = F.below(s);
    if(bl.empty()) continue;
    const int p = F.sn_of_b[bl[0]];
    if(S.sn_level[p] < S.sn_level[s] + 1) S.sn_level[p] = S.sn_level[s] + 1;
  }
  S.nlevels = 0;
  for(int s = 0; s < nsn; s++) S.nlevels = std::max(S.nlevels, S.sn_level[s] + 1);
  S.lvl_ptr.assign(S.nlevels + 1, 0);
  for(int s = 0; s < nsn; s++) S.lvl_ptr[S.sn_level[s] + 1]++;
  for(int l = 0; l < S.nlevels; l++) S.lvl_ptr[l+1] += S.lvl_ptr[l];
  S.lvl_sn.resize(nsn);
  {
    std::vector<int> nx(S.lvl_ptr.begin(), S.lvl_ptr.end() - 1);
    for(int s = 0; s < nsn; s++) S.lvl_sn[nx[S.sn_level[s]]++] = s;
  }
  F.sn_parent0.assign(nsn, -1);
  for(int d = 0; d < nsn; d++) { const std::vector<int>& bl = F.below(d); if(!bl.empty()) F.sn_parent0[d] = F.sn_of_b[bl[0]]; }
}

// ---- subtree partition (multi-GPU, SURVEY 8e "point ownership"): the elimination tree is cut
// above level `cut_level`; every subtree below the cut belongs to ONE rank, which holds the
// measurement rows whose first-eliminated variable lies in it, assembles, factors and solves it
// alone -- a row's variables are a clique of JtJ, so they all sit on one root path and a subtree's
// panels receive contributions from its owner's rows only.  The supernodes above the cut are
// replicated: their panels (assembled entries + the owners' updates, both partial sums) and the
// update matrices handed up across the cut are summed over the ranks once per factorisation.
void sym_partition(int part_nranks, SymFront& F, SymHost& S)
{
  const int nvb = F.nvb, nrb = F.nrb, nsn = F.nsn, part_rank = F.part_rank;
  const bool partition = part_nranks > 1;
  S.sn_owner.assign(nsn, -1);
  S.cut_level = -1;
  if(partition)
  {
    const int oversub = 1;
    for(int l = S.nlevels - 1; l >= 0; l--)
      if(S.lvl_ptr[l+1] - S.lvl_ptr[l] >= part_nranks*oversub) { S.cut_level = l; break; }
    const int Lc = S.cut_level;
    // weight of a subtree: panel entries (a proxy for its assembly, factorisation and solve work)
    std::vector<double> wt(nsn, 0.0);
    for(int d = 0; d < nsn; d++)
    {
      wt[d] += (double)(S.sn_rowptr[d+1] - S.sn_rowptr[d])*(S.sn_c0[d+1] - S.sn_c0[d]);
      if(F.sn_parent0[d] >= 0 && S.sn_level[F.sn_parent0[d]] <= Lc) wt[F.sn_parent0[d]] += wt[d];     // parents come later
    }
    std::vector<int> roots;
    for(int d = 0; d < nsn; d++)
      if(S.sn_level[d] <= Lc && (F.sn_parent0[d] < 0 || S.sn_level[F.sn_parent0[d]] > Lc)) roots.push_back(d);
    std::sort(roots.begin(), roots.end(), [&](int a, int b) { if(wt[a] != wt[b]) return wt[a] > wt[b]; return a < b; });
    std::vector<double> load(part_nranks, 0.0);
    for(int d : roots)
    {
      int best = 0;
      for(int r = 1; r < part_nranks; r++) if(load[r] < load[best]) best = r;
      S.sn_owner[d] = best; load[best] += wt[d];
    }
    for(int d = nsn - 1; d >= 0; d--)
      if(S.sn_level[d] <= Lc && S.sn_owner[d] < 0) S.sn_owner[d] = S.sn_owner[F.sn_parent0[d]];
    // rows: the row-blocks whose first-eliminated variable lies in one of this rank's subtrees; rows
    // that only touch replicated variables are dealt out in turn
    int lb = 0, lr = 0, turn = 0;
    S.part_rows.clear();
    for(int bi = 0; bi < nrb; bi++)
    {
      RowBlock& b = F.rbs[bi];
      int qmin = nvb;
      for(int x = 0; x < b.nvb; x++) qmin = std::min(qmin, F.bpos[F.rb_vb[b.vptr + x]]);
      int own = S.sn_owner[F.sn_of_b[qmin]];
      if(own < 0) own = (turn++) % part_nranks;
      b.local = own == part_rank;
      b.lbase = lb; b.lr0 = lr;
      if(b.local) { lb += b.nrows*b.len; lr += b.nrows; for(int r = 0; r < b.nrows; r++) S.part_rows.push_back(b.r0 + r); }
    }
  }
  // the supernodes this rank works on, by level (all of them on a single rank)
  S.xl_ptr.assign(S.nlevels + 1, 0);
  S.xl_sn.clear();
  for(int l = 0; l < S.nlevels; l++)
  {
    for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1]; i++) if(F.mine(S, S.lvl_sn[i])) S.xl_sn.push_back(S.lvl_sn[i]);
    S.xl_ptr[l+1] = (int)S.xl_sn.size();
  }
}

// factor work list: (supernode, slice of its below rows).  Panels larger than the LDS
// budget are cut into row slices; every slice workgroup also holds the w x w top block
// and factors it redundantly, only slice 0 publishes it (into top_scr, copied back at
// the end: no other kernel of the factorisation reads a top block).
void sym_factor_work_list(const SymFront& F, const SymKnobs& K, SymHost& S)
{
  const int nsn = F.nsn;
  S.fw_lvl_ptr.assign(S.nlevels + 1, 0);
  S.sn_top.assign(nsn, -1);
  S.top_size = 0;
  for(int l = 0; l < S.nlevels; l++)
  {
    for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1]; i++)
    {
      const int s = S.lvl_sn[i];
      const int w = S.sn_c0[s+1] - S.sn_c0[s];
      const int nrows = S.sn_rowptr[s+1] - S.sn_rowptr[s];
      const int below = nrows - w;
      int nsl = 1;
      if((long)((nrows + 1) & ~1)*w > K.slice_cap)
      {
        int rpw = K.slice_cap/w - w - 1; if(rpw < 1) rpw = 1;
        nsl = (below + rpw - 1)/rpw;
      }
      // (the slicing of every supernode is recorded -- it decides where the multifrontal region
      // starts, identically on every rank --, work items only for this rank's supernodes)
      if(nsl > 1) { S.sn_top[s] = S.top_size; S.top_size += (int64_t)w*w; if(F.mine(S, s)) S.ms_sn.push_back(s); }
      if(!F.mine(S, s)) continue;
      const int per = (below + nsl - 1)/nsl;
      for(int k = 0; k < nsl; k++)
      {
        S.fw_sn.push_back(s); S.fw_r0.push_back(std::min(below, k*per)); S.fw_r1.push_back(std::min(below, (k+1)*per));
      }
      S.fw_lvl_ptr[l+1] += nsl;
    }
  }
  for(int l = 0; l < S.nlevels; l++) S.fw_lvl_ptr[l+1] += S.fw_lvl_ptr[l];
}

// DOGLEG_AMD_SYM_DEBUG: the supernodes of every level on stderr
void sym_level_dump(const SymHost& S)
{
  for(int l = 0; l < S.nlevels; l++)
  {
    long n = 0, wsum = 0, rsum = 0, nofit = 0; int wmin = 1 << 30, wmax = 0, rmax = 0;
    for(int i = S.lvl_ptr[l]; i < S.lvl_ptr[l+1]; i++)
    {
      const int s = S.lvl_sn[i];
      const int w = S.sn_c0[s+1] - S.sn_c0[s], nr = S.sn_rowptr[s+1] - S.sn_rowptr[s];
      n++; wsum += w; rsum += nr; wmin = std::min(wmin, w); wmax = std::max(wmax, w); rmax = std::max(rmax, nr);
      if(sym_w_split(w, nr) < 0) nofit++;
    }
    fprintf(stderr, "level %2d: %5ld supernodes  w min/avg/max %d/%.1f/%d  nrows avg/max %.1f/%d  slices %d  update matrix not in LDS: %ld\n", l, n, wmin,
            (double)wsum/n, wmax, (double)rsum/n, rmax, S.fw_lvl_ptr[l+1] - S.fw_lvl_ptr[l], nofit);
  }
}

} // namespace

// ------------------------------------------- 9a. Jt*x lists (per var-block)
void sym_jtx_lists(const SymHost& S, const SymFront& F, SymJtx& R)
{
  const int nvb = F.nvb, nrb = F.nrb;
  // inverted index: var-block -> local row-blocks containing it (row order)
  std::vector<int> rptr(nvb + 1, 0);
  for(const RowBlock& b : F.rbs) if(b.local) for(int x = 0; x < b.nvb; x++) rptr[F.rb_vb[b.vptr + x] + 1]++;
  for(int v = 0; v < nvb; v++) rptr[v+1] += rptr[v];
  R.oblk.resize(nvb);
  R.contrib.resize(rptr[nvb]);
  std::vector<int> nx(rptr.begin(), rptr.end() - 1);
  for(int bi = 0; bi < nrb; bi++)
  {
    const RowBlock& b = F.rbs[bi];
    if(!b.local) continue;
    for(int x = 0; x < b.nvb; x++)
    {
      SymContrib c; c.base = b.lbase; c.r0 = b.lr0; c.len = (uint16_t)b.len;
      c.nrows = (uint8_t)b.nrows; c.pad = 0; c.offI = c.offJ = (uint16_t)F.rb_off[b.vptr + x];
      R.contrib[nx[F.rb_vb[b.vptr + x]]++] = c;
    }
  }
  for(int v = 0; v < nvb; v++)
  {
    const int q = F.bpos[v], t = F.sn_of_b[q];
    const int ld = S.sn_rowptr[t+1] - S.sn_rowptr[t];
    const int lc = F.colstart[q] - S.sn_c0[t];
    SymOutBlock o; memset(&o, 0, sizeof(o));
    o.dest = S.sn_lx[t] + lc + (int64_t)lc*ld; o.ld = ld; o.var0 = S.vb_start[v];
    o.nI = o.nJ = (uint8_t)F.w[v]; o.diag = 1;
    R.oblk[v] = o;
  }
  R.jtx_nparts = 0; R.jtx_fin_ptr.assign(1, 0); R.jtx_fin_blk.clear();
  R.jtx_covers_all = true;
  for(int v = 0; v < nvb; v++)
  {
    const int c0 = rptr[v], c1 = rptr[v+1];
    if(c1 == c0) { R.jtx_covers_all = false; continue; }
    int chunk = CH_JTX;
    if((c1 - c0 + chunk - 1)/chunk > MAXCH_JTX) chunk = (c1 - c0 + MAXCH_JTX - 1)/MAXCH_JTX;
    const int nch = (c1 - c0 + chunk - 1)/chunk;
    if(nch == 1) R.jtx_task.push_back({v, c0, c1, -1, S.vb_start[v], F.w[v]});
    else
    {
      for(int k = 0; k < nch; k++)
        R.jtx_task.push_back({v, c0 + k*chunk, std::min(c1, c0 + (k+1)*chunk), R.jtx_nparts + k, S.vb_start[v], F.w[v]});
      R.jtx_nparts += nch;
      R.jtx_fin_blk.push_back(v); R.jtx_fin_ptr.push_back(R.jtx_nparts);
    }
  }
}

// --------------------------------------- 10. forward-solve gather lists
void sym_solve_gather(const SymHost& S, SymGather& R)
{
  const int N = S.N, nsn = S.nsn;
  R.rl_ptr.assign(N + 1, 0);
  for(int d = 0; d < nsn; d++)
  {
    const int wd = S.sn_c0[d+1] - S.sn_c0[d];
    for(int k = S.sn_rowptr[d] + wd; k < S.sn_rowptr[d+1] - 1; k++) R.rl_ptr[S.sn_rows[k] + 1]++;
  }
  for(int k = 0; k < N; k++) R.rl_ptr[k+1] += R.rl_ptr[k];
  R.rl_pos.resize(R.rl_ptr[N]);
  std::vector<int> nx(R.rl_ptr.begin(), R.rl_ptr.end() - 1);
  for(int d = 0; d < nsn; d++)
  {
    const int wd = S.sn_c0[d+1] - S.sn_c0[d];
    for(int k = S.sn_rowptr[d] + wd, j = 0; k < S.sn_rowptr[d+1] - 1; k++, j++)
      R.rl_pos[nx[S.sn_rows[k]]++] = S.sn_scr[d] + j;
  }
}

void SymJtx::into(SymHost& S)
{
  S.oblk = std::move(oblk);
  S.contrib = std::move(contrib);
  S.jtx_task = std::move(jtx_task);
  S.jtx_fin_ptr = std::move(jtx_fin_ptr);
  S.jtx_fin_blk = std::move(jtx_fin_blk);
  S.jtx_nparts = jtx_nparts;
  S.jtx_covers_all = jtx_covers_all;
}

void SymGather::into(SymHost& S)
{
  S.rl_ptr = std::move(rl_ptr);
  S.rl_pos = std::move(rl_pos);
}

int sym_analyze(SymHost& S, int N, int M, const int* cp, const int* ri, int row0, int row1,
                char* err, int errlen, int part_rank, int part_nranks)
{
  const SymKnobs K = sym_knobs_env();
  const bool partition = part_nranks > 1;
  if(partition) { row0 = 0; row1 = M; }           // the rows of a rank are chosen below, not given
  // DOGLEG_AMD_SYM_DEBUG >= 2: wall time of every step on stderr
  auto sym_t0 = std::chrono::steady_clock::now();
  const char* sym_what = "setup";
  auto sym_tick = [&](const char* next) {
    if(K.debug >= 2)
    {
      const auto t1 = std::chrono::steady_clock::now();
      fprintf(stderr, "sym_analyze: %-40s %8.1f ms\n", sym_what, std::chrono::duration<double, std::milli>(t1 - sym_t0).count());
      sym_t0 = t1;
    }
    sym_what = next; };

  S = SymHost();
  S.N = N; S.M = M; S.nnz = cp[M]; S.row0 = row0; S.row1 = row1;
  S.part_rank = partition ? part_rank : 0; S.part_nranks = partition ? part_nranks : 1;
  if(cp[0] != 0) SYM_FAIL("Jt column pointers must start at 0");

  SymFront F;
  F.part_rank = part_rank;
  std::vector<int> vb_of;               // variable -> var-block
  Graph G;
  BlockTree T;
  std::vector<char> sn_bd;
  sym_tick("1 var-blocks");
  if(sym_var_blocks(N, M, cp, ri, S, F, vb_of, err, errlen)) return 1;
  sym_tick("2 row-blocks");
  sym_row_blocks(M, cp, ri, row0, row1, vb_of, S, F);
  sym_tick("3 block graph of JtJ");
  sym_block_graph(F, G, S.nnz_JtJ_lower);
  sym_tick("4 ordering");
  if(sym_ordering(G, K, F, err, errlen)) return 1;
  sym_tick("5 block-level symbolic factorisation");
  if(sym_block_factor(G, F, T, S, err, errlen)) return 1;
  sym_tick("6 supernodes");
  sym_supernodes(T, K, F, sn_bd);
  sym_tick("7 scalar-level layout");
  sym_layout(T, sn_bd, F, S);
  sym_partition(part_nranks, F, S);
  sym_factor_work_list(F, K, S);
  if(K.debug) sym_level_dump(S);

  // steps 8, 9a, 9b and 10 on four threads: each reads S, F and K through const references and fills a record of its own
  sym_tick("8-10 schedules (4 threads)");
  SymUpdate u8; SymJtx j9a; SymAssembly a9b; SymGather g10;
  char e8[256] = "", e9b[256] = "";
  int r8 = 0;
  std::thread t8([&] { r8 = sym_update_schedule(S, F, K, u8, e8, sizeof(e8)); });
  std::thread t9a([&] { sym_jtx_lists(S, F, j9a); });
  std::thread t10([&] { sym_solve_gather(S, g10); });
  const int r9b = sym_assembly_schedule(S, F, K, a9b, e9b, sizeof(e9b));
  t8.join(); t9a.join(); t10.join();
  if(r8 || r9b) SYM_FAIL("%s", r8 ? e8 : e9b);
  u8.into(S); j9a.into(S); a9b.into(S); g10.into(S);
  sym_tick("done");
  return 0;
}
