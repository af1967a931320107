// Python bindings for the NornicDB-AMD native kernel library (_C).
#include <torch/extension.h>

// vector_ops.hip
void l2_normalize_(at::Tensor x);
void fill_random_unit_(at::Tensor x, long long row_base, long long seed);

// knn_gemv.hip
std::tuple<at::Tensor, at::Tensor> knn_gemv(at::Tensor db, at::Tensor q,
                                            long long row_base, int k_out,
                                            c10::optional<at::Tensor> allow,
                                            c10::optional<at::Tensor> row_bias);

// ivf_scan.hip
std::tuple<at::Tensor, at::Tensor> ivf_scan(
    at::Tensor db, at::Tensor q, at::Tensor probes, at::Tensor list_off,
    at::Tensor list_rows, long long tail_start, long long max_len,
    long long row_base, int k_out, c10::optional<at::Tensor> allow);
std::tuple<at::Tensor, at::Tensor> ivf_scan_i8(
    at::Tensor db, at::Tensor sa, at::Tensor q, at::Tensor sq,
    at::Tensor probes, at::Tensor list_off, at::Tensor list_rows,
    long long tail_start, long long max_len, long long row_base, int k_out,
    c10::optional<at::Tensor> allow);
std::tuple<at::Tensor, at::Tensor> ivf_scan_fp8(
    at::Tensor db, at::Tensor q, at::Tensor probes, at::Tensor list_off,
    at::Tensor list_rows, long long tail_start, long long max_len,
    long long row_base, int k_out, c10::optional<at::Tensor> allow);

// bm25_scan.hip
long long bm25_range_value();
std::tuple<at::Tensor, at::Tensor> bm25_scan(
    at::Tensor post_off, at::Tensor post_doc, at::Tensor post_tf,
    at::Tensor doc_len, at::Tensor q_terms, at::Tensor q_w, double c0,
    double c1, int k_out, c10::optional<at::Tensor> allow);

// knn_mfma.hip
long long knn_bm_value();
long long knn_rg_value();
long long knn_stagger_value();
#define KNN_BM_VALUE knn_bm_value()
std::tuple<at::Tensor, at::Tensor> knn_mfma(at::Tensor db, at::Tensor q,
                                            long long row_base, int k_out,
                                            c10::optional<at::Tensor> allow,
                                            c10::optional<at::Tensor> row_bias,
                                            int q_count);

// knn_q8.hip
long long knn_q8_bm_value();
std::tuple<at::Tensor, at::Tensor> knn_fp8(at::Tensor db, at::Tensor q,
                                           long long row_base, int k_out,
                                           c10::optional<at::Tensor> allow);
std::tuple<at::Tensor, at::Tensor> knn_i8(at::Tensor db, at::Tensor sa,
                                          at::Tensor q, at::Tensor sq,
                                          long long row_base, int k_out,
                                          c10::optional<at::Tensor> allow);

// gemm.hip
at::Tensor gemm_nt(at::Tensor a, at::Tensor w, c10::optional<at::Tensor> bias,
                   long long act);
long long gemm_nt_variant(long long M);

// kmeans.hip
std::tuple<at::Tensor, at::Tensor> kmeans_assign(at::Tensor x, at::Tensor cent,
                                                 at::Tensor cnorm2);
std::tuple<at::Tensor, at::Tensor> kmeans_accum(at::Tensor x, at::Tensor assign,
                                                long long k);
std::tuple<at::Tensor, at::Tensor> kmeans_finalize(at::Tensor sums,
                                                   at::Tensor counts,
                                                   at::Tensor old_c);
void kmeanspp_update(at::Tensor x, at::Tensor c, double cn2, at::Tensor d2);
void kmeans_point_update(at::Tensor cent, at::Tensor counts, at::Tensor xv,
                         long long c, long long sign);

// graph.hip
at::Tensor pagerank_contrib(at::Tensor rank, at::Tensor outdeg);
at::Tensor pagerank_gather(at::Tensor row_ptr, at::Tensor col_idx,
                           at::Tensor contrib, double damping, double base);
void bfs_level(at::Tensor row_ptr, at::Tensor col_idx, at::Tensor dist,
               at::Tensor changed, long long row_base, long long level);
at::Tensor labelprop_step(at::Tensor row_ptr, at::Tensor col_idx,
                          at::Tensor labels, at::Tensor changed,
                          long long row_base);
void wcc_hook(at::Tensor row_ptr, at::Tensor col_idx, at::Tensor comp,
              at::Tensor changed, long long row_base);

// centrality.hip
void msbfs_level(at::Tensor in_row_ptr, at::Tensor in_col_idx,
                 at::Tensor frontier, at::Tensor visited, at::Tensor next,
                 at::Tensor level_count, long long full_mask);
void bc_forward(at::Tensor in_row_ptr, at::Tensor in_col_idx, at::Tensor dist,
                at::Tensor sigma, at::Tensor changed, long long level);
void bc_backward(at::Tensor row_ptr, at::Tensor col_idx, at::Tensor dist,
                 at::Tensor sigma, at::Tensor delta, long long level);
void bc_accumulate(at::Tensor delta, at::Tensor sources, at::Tensor bc);

// packstream.cpp (CPU)
pybind11::bytes ps_pack(pybind11::object v);
pybind11::object ps_unpack(pybind11::buffer data,
                           pybind11::object structure_factory);

// encoder_ops.hip
at::Tensor add_layernorm(at::Tensor a, c10::optional<at::Tensor> b,
                         at::Tensor gamma, at::Tensor beta, double eps);
at::Tensor bias_gelu(at::Tensor x, at::Tensor bias);
at::Tensor mean_pool_l2norm(at::Tensor x, c10::optional<at::Tensor> mask);

// flash_attn.hip
at::Tensor flash_attn_nc(at::Tensor q, at::Tensor k, at::Tensor v);

// decode_fused.hip
void decode_step(at::Tensor layer_ptrs, at::Tensor x, at::Tensor q,
                 at::Tensor attn, at::Tensor h, at::Tensor rope_cos,
                 at::Tensor rope_sin, long long n_layers, long long hidden,
                 long long n_heads, long long n_kv, long long hd,
                 long long inter, long long max_len, double rms_eps,
                 long long pos);
double sync_bench(long long iters, long long which, long long grid,
                  at::Tensor scratch);
void decode_tokens(at::Tensor layer_ptrs, at::Tensor x, at::Tensor q,
                   at::Tensor attn, at::Tensor h, at::Tensor rope_cos,
                   at::Tensor rope_sin, at::Tensor embed_w,
                   at::Tensor norm_w, at::Tensor lm_w, at::Tensor out,
                   at::Tensor n_done, at::Tensor pmax, at::Tensor pidx,
                   long long n_layers, long long hidden, long long n_heads,
                   long long n_kv, long long hd, long long inter,
                   long long max_len, double rms_eps, long long pos,
                   long long start_tok, long long n_toks, long long eos);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "NornicDB-AMD CDNA4 (gfx950) native kernels";
  m.def("l2_normalize_", &l2_normalize_, "In-place row L2 normalize (bf16/f32)");
  m.def("fill_random_unit_", &fill_random_unit_,
        "Fill with deterministic unit-norm pseudo-gaussian rows (bf16)",
        py::arg("x"), py::arg("row_base") = 0, py::arg("seed") = 0x6e6f726eLL);
  m.def("knn_gemv", &knn_gemv,
        "Fused cosine score + top-k for <=16 queries (bf16 db); allow = "
        "optional packed int32 row mask (bit r&31 of word r>>5); row_bias = "
        "optional fp32 [N] added to each row's score",
        py::arg("db"), py::arg("q"), py::arg("row_base") = 0,
        py::arg("k_out") = 10, py::arg("allow") = c10::nullopt,
        py::arg("row_bias") = c10::nullopt);
  m.def("ivf_scan", &ivf_scan,
        "IVF probe-list scan: fused gather + cosine score + top-k (k <= 64) "
        "over the probed inverted lists and the unclustered tail (bf16 db)",
        py::arg("db"), py::arg("q"), py::arg("probes"), py::arg("list_off"),
        py::arg("list_rows"), py::arg("tail_start"), py::arg("max_len"),
        py::arg("row_base") = 0, py::arg("k_out") = 10,
        py::arg("allow") = c10::nullopt);
  m.def("ivf_scan_i8", &ivf_scan_i8,
        "IVF probe-list scan over a symmetric int8 corpus with per-row "
        "scales (score = i32 dot * sa[row] * sq[query]); q is the int8 "
        "query, sq its scales",
        py::arg("db"), py::arg("sa"), py::arg("q"), py::arg("sq"),
        py::arg("probes"), py::arg("list_off"), py::arg("list_rows"),
        py::arg("tail_start"), py::arg("max_len"), py::arg("row_base") = 0,
        py::arg("k_out") = 10, py::arg("allow") = c10::nullopt);
  m.def("ivf_scan_fp8", &ivf_scan_fp8,
        "IVF probe-list scan over an FP8 e4m3fn corpus (uint8 carrier for "
        "db and q), fp32 accumulation",
        py::arg("db"), py::arg("q"), py::arg("probes"), py::arg("list_off"),
        py::arg("list_rows"), py::arg("tail_start"), py::arg("max_len"),
        py::arg("row_base") = 0, py::arg("k_out") = 10,
        py::arg("allow") = c10::nullopt);
  // BM25_RANGE: documents per LDS accumulator range of bm25_scan
  m.attr("BM25_RANGE") = bm25_range_value();
  m.def("bm25_scan", &bm25_scan,
        "BM25 posting-list scan: fused posting gather + score + top-k "
        "(k <= 64) over CSR postings; a posting adds w*tf/(tf+c0+c1*dl) to "
        "its document, only documents with a score > 0 are returned",
        py::arg("post_off"), py::arg("post_doc"), py::arg("post_tf"),
        py::arg("doc_len"), py::arg("q_terms"), py::arg("q_w"),
        py::arg("c0"), py::arg("c1"), py::arg("k_out") = 10,
        py::arg("allow") = c10::nullopt);
  // KNN_BM: rows of one kNN panel; KNN_RG: row groups the panel is made of
  m.attr("KNN_BM") = KNN_BM_VALUE;
  m.attr("KNN_RG") = knn_rg_value();
  // KNN_STAGGER: 1 when row group 1 runs half a stage behind row group 0
  m.attr("KNN_STAGGER") = knn_stagger_value();
  m.def("knn_mfma", &knn_mfma,
        "Fused MFMA cosine score + top-k, 256-query batches (bf16 db); "
        "row_bias = optional fp32 [N] added to each row's score; q_count = "
        "real queries among the 256 rows of q (with row_bias the padding "
        "columns are not scored; their output rows are undefined)",
        py::arg("db"), py::arg("q"), py::arg("row_base") = 0,
        py::arg("k_out") = 10, py::arg("allow") = c10::nullopt,
        py::arg("row_bias") = c10::nullopt, py::arg("q_count") = 256);
  m.def("gemm_nt", &gemm_nt,
        "C = A[M,K] @ W[N,K]^T + bias (+GELU), bf16 MFMA; kernel per "
        "gemm_nt_variant(M)",
        py::arg("a"), py::arg("w"), py::arg("bias") = c10::nullopt,
        py::arg("act") = 0);
  m.def("gemm_nt_variant", &gemm_nt_variant,
        "row tile (96 or 256) of the kernel gemm_nt launches for M rows, "
        "NORNICDB_GEMM_KERNEL honoured as in the launch",
        py::arg("m"));
  m.def("add_layernorm", &add_layernorm, "LN(a+b)*gamma+beta fused (bf16)",
        py::arg("a"), py::arg("b"), py::arg("gamma"), py::arg("beta"),
        py::arg("eps") = 1e-5);
  m.def("bias_gelu", &bias_gelu, "gelu(x+bias) fused (bf16)");
  m.def("mean_pool_l2norm", &mean_pool_l2norm,
        "masked mean-pool + L2 norm (bf16 -> fp32)",
        py::arg("x"), py::arg("mask") = c10::nullopt);
  m.def("flash_attn_nc", &flash_attn_nc,
        "non-causal flash attention fwd, head_dim 64 (bf16)");
  m.def("decode_step", &decode_step,
        "fused cooperative single-token decode (all layers, one launch)",
        py::arg("layer_ptrs"), py::arg("x"), py::arg("q"), py::arg("attn"),
        py::arg("h"), py::arg("rope_cos"), py::arg("rope_sin"),
        py::arg("n_layers"), py::arg("hidden"), py::arg("n_heads"),
        py::arg("n_kv"), py::arg("hd"), py::arg("inter"),
        py::arg("max_len"), py::arg("rms_eps"), py::arg("pos"));
  m.def("decode_tokens", &decode_tokens,
        "fused cooperative multi-token greedy decode (embed + layers + "
        "lm_head argmax, whole generation loop in one launch)",
        py::arg("layer_ptrs"), py::arg("x"), py::arg("q"), py::arg("attn"),
        py::arg("h"), py::arg("rope_cos"), py::arg("rope_sin"),
        py::arg("embed_w"), py::arg("norm_w"), py::arg("lm_w"),
        py::arg("out"), py::arg("n_done"), py::arg("pmax"), py::arg("pidx"),
        py::arg("n_layers"), py::arg("hidden"), py::arg("n_heads"),
        py::arg("n_kv"), py::arg("hd"), py::arg("inter"),
        py::arg("max_len"), py::arg("rms_eps"), py::arg("pos"),
        py::arg("start_tok"), py::arg("n_toks"), py::arg("eos") = -1);
  // KNN_Q8_BM: rows of one panel of the quantised (int8 / fp8) kNN kernel
  m.attr("KNN_Q8_BM") = knn_q8_bm_value();
  m.def("knn_i8", &knn_i8,
        "Fused i8 MFMA score + top-k over a symmetric int8 corpus with "
        "per-row scales (score = i32 dot * sa[row] * sq[col])",
        py::arg("db"), py::arg("sa"), py::arg("q"), py::arg("sq"),
        py::arg("row_base") = 0, py::arg("k_out") = 10,
        py::arg("allow") = c10::nullopt);
  m.def("knn_fp8", &knn_fp8,
        "Fused MFMA cosine score + top-k over an FP8 e4m3fn corpus "
        "(uint8 carrier), 256-query batches",
        py::arg("db"), py::arg("q"), py::arg("row_base") = 0,
        py::arg("k_out") = 10, py::arg("allow") = c10::nullopt);
  m.def("sync_bench", &sync_bench,
        "grid-barrier microbenchmark: ms for `iters` barriers "
        "(which=0 cg::grid.sync, 1 two-level custom)",
        py::arg("iters"), py::arg("which"), py::arg("grid"),
        py::arg("scratch"));
  m.def("kmeans_assign", &kmeans_assign,
        "fused distance+argmin assignment (bf16 x/centroids)");
  m.def("kmeans_accum", &kmeans_accum,
        "atomic centroid accumulate. assign values must lie in [0, k): the "
        "wrapper cannot check them without a device sync, and a value "
        "outside is an out-of-bounds write");
  m.def("kmeans_finalize", &kmeans_finalize,
        "sums/counts -> centroids + drift^2 (empty keep old)");
  m.def("kmeanspp_update", &kmeanspp_update,
        "d2 = min(d2, dist2(x, new_seed))");
  m.def("kmeans_point_update", &kmeans_point_update,
        "incremental single-point centroid update (+1 add / -1 remove)");
  m.def("pagerank_contrib", &pagerank_contrib, "rank/outdeg elementwise");
  m.def("pagerank_gather", &pagerank_gather,
        "CSR pull-gather pagerank iteration (wave per row)");
  m.def("bfs_level", &bfs_level, "BFS frontier level expansion");
  m.def("labelprop_step", &labelprop_step, "label propagation step");
  m.def("wcc_hook", &wcc_hook, "connected-components hook step");
  m.def("msbfs_level", &msbfs_level,
        "multi-source BFS level over the in-edge CSR, 64 sources per uint64 "
        "word (held as int64): next = OR frontier[in-nbrs] & ~visited, "
        "visited |= next, level_count[64] += newly reached per source bit");
  m.def("bc_forward", &bc_forward,
        "Brandes forward level over the in-edge CSR for dist/sigma [B][n]");
  m.def("bc_backward", &bc_backward,
        "Brandes backward level over the out-edge CSR for delta [B][n]");
  m.def("bc_accumulate", &bc_accumulate,
        "bc[v] += delta[b][v] for b in order, skipping v == sources[b]");
  m.def("ps_pack", &ps_pack, "PackStream encode (native)");
  m.def("ps_unpack", &ps_unpack, "PackStream decode (native)",
        py::arg("data"), py::arg("structure_factory"));
}
