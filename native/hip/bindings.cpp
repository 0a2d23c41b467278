// pybind11 module `_hip`: device query, CU-masked streams, XCD probe, load kernels,
// xGMI probes.  All device pointers / streams cross the boundary as integers
// (torch.Tensor.data_ptr(), torch.cuda.Stream.cuda_stream), so the module does not link
// libtorch and builds in seconds with hipcc.
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "api.h"

namespace py = pybind11;

PYBIND11_MODULE(_hip, m) {
  m.doc() = "MI355X native HIP layer (gfx950)";
  m.attr("ARCH") = "gfx950";
  m.def("device_count", &gs::device_count);
  m.def("query_all", []() {
    py::list out;
    for (auto& d : gs::query_all()) {
      py::dict x;
      x["index"] = d.index;
      x["name"] = d.name;
      x["arch"] = d.arch;
      x["uuid"] = d.uuid;
      x["rocr_uuid"] = d.rocr_uuid;
      x["pci"] = d.pci;
      x["cus"] = d.cus;
      x["clock_khz"] = d.clock_khz;
      x["mem_clock_khz"] = d.mem_clock_khz;
      x["warp"] = d.warp;
      x["l2_bytes"] = d.l2_bytes;
      x["max_threads"] = d.max_threads;
      x["lds_per_block"] = d.lds_per_block;
      x["total_mem"] = d.total_mem;
      x["free_mem"] = d.free_mem;
      x["heap_limit"] = d.heap_limit;
      x["fifo_limit"] = d.fifo_limit;
      x["stack_limit"] = d.stack_limit;
      out.append(x);
    }
    return out;
  });
  m.def("create_masked_stream", &gs::create_masked_stream, py::arg("mask"));
  m.def("create_stream", &gs::create_stream, py::arg("priority") = 0);
  m.def("destroy_stream", &gs::destroy_stream);
  m.def("get_stream_mask", &gs::get_stream_mask);
  m.def("probe_xcd", &gs::probe_xcd, py::arg("stream"), py::arg("n"));
  m.def("gemm_bf16_nt", &gs::gemm_bf16_nt, py::arg("a"), py::arg("bt"), py::arg("c"), py::arg("bias"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("relu"),
        py::arg("stream"), py::arg("cu_budget") = 0, py::arg("workspace") = 0, py::arg("workspace_floats") = 0,
        py::call_guard<py::gil_scoped_release>());
  m.def("pick_split_k", &gs::pick_split_k, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("cu_budget") = 0);
  m.def("splitk_workspace_floats", &gs::splitk_workspace_floats, py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("cu_budget") = 0);
  m.def("gemm_fp8_nt", &gs::gemm_fp8_nt, py::arg("a"), py::arg("bt"), py::arg("c"), py::arg("bias"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("relu"),
        py::arg("stream"), py::arg("cu_budget") = 0, py::call_guard<py::gil_scoped_release>());
  m.def("stream_triad", &gs::stream_triad, py::arg("a"), py::arg("b"), py::arg("c"), py::arg("s"),
        py::arg("n_floats"), py::arg("blocks"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("embedding_bag_bf16", &gs::embedding_bag_bf16, py::arg("table"), py::arg("idx"), py::arg("offsets"),
        py::arg("out"), py::arg("B"), py::arg("D"), py::arg("ld_table"), py::arg("ld_out"), py::arg("blocks"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("embedding_bag_workgroups", &gs::embedding_bag_workgroups, py::arg("B"), py::arg("blocks") = 0);
  m.def("paged_decode_bf16", &gs::paged_decode_bf16, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_table"), py::arg("ctx_lens"), py::arg("out"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"),
        py::arg("ld_q"), py::arg("ld_out"), py::arg("ld_table"), py::arg("scale"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("paged_decode_workgroups", &gs::paged_decode_workgroups, py::arg("S"), py::arg("Hkv"));
  m.def("paged_decode_split_bf16", &gs::paged_decode_split_bf16, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_table"), py::arg("ctx_lens"), py::arg("workspace"), py::arg("out"), py::arg("S"), py::arg("Hq"),
        py::arg("Hkv"), py::arg("kv_splits"), py::arg("ld_q"), py::arg("ld_out"), py::arg("ld_table"),
        py::arg("scale"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("paged_decode_split_workgroups", &gs::paged_decode_split_workgroups, py::arg("S"), py::arg("Hkv"),
        py::arg("kv_splits"));
  m.def("paged_decode_split_workspace_floats", &gs::paged_decode_split_workspace_floats, py::arg("S"), py::arg("Hq"),
        py::arg("kv_splits"));
  m.def("paged_prefill_bf16", &gs::paged_prefill_bf16, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("block_table"), py::arg("ctx_lens"), py::arg("q_start"), py::arg("out"), py::arg("S"), py::arg("Hq"),
        py::arg("Hkv"), py::arg("max_q_len"), py::arg("ld_q"), py::arg("ld_out"), py::arg("ld_table"), py::arg("scale"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("paged_prefill_workgroups", &gs::paged_prefill_workgroups, py::arg("S"), py::arg("Hq"), py::arg("Hkv"),
        py::arg("max_q_len"));
  m.def("rope_append_bf16", &gs::rope_append_bf16, py::arg("qkv"), py::arg("cos_sin"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("block_table"), py::arg("ctx_lens"), py::arg("q_start"), py::arg("q_out"),
        py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("max_q_len"), py::arg("max_pos"), py::arg("ld_qkv"),
        py::arg("ld_q_out"), py::arg("ld_table"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("rope_append_workgroups", &gs::rope_append_workgroups, py::arg("S"), py::arg("Hkv"), py::arg("max_q_len"));
  m.def("add_rmsnorm_bf16", &gs::add_rmsnorm_bf16, py::arg("x"), py::arg("residual"), py::arg("weight"),
        py::arg("res_out"), py::arg("y"), py::arg("T"), py::arg("D"), py::arg("ld_x"), py::arg("ld_res"),
        py::arg("ld_res_out"), py::arg("ld_y"), py::arg("eps"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("add_rmsnorm_workgroups", &gs::add_rmsnorm_workgroups, py::arg("T"));
  m.def("swiglu_bf16", &gs::swiglu_bf16, py::arg("gate_up"), py::arg("out"), py::arg("T"), py::arg("F"),
        py::arg("ld_in"), py::arg("ld_out"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("swiglu_workgroups", &gs::swiglu_workgroups, py::arg("T"), py::arg("F"));
  m.def("sample_topk_bf16", &gs::sample_topk_bf16, py::arg("logits"), py::arg("u"), py::arg("temperature"),
        py::arg("top_k"), py::arg("top_p"), py::arg("out"), py::arg("S"), py::arg("V"), py::arg("ld_logits"),
        py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("sample_workgroups", &gs::sample_workgroups, py::arg("S"));
  m.def("moe_max_tiles", &gs::moe_max_tiles, py::arg("T"), py::arg("k"), py::arg("E"));
  m.def("moe_route_bf16", &gs::moe_route_bf16, py::arg("logits"), py::arg("topk_ids"), py::arg("topk_w"),
        py::arg("sorted_ids"), py::arg("tile_expert"), py::arg("expert_offsets"), py::arg("slot_pos"), py::arg("T"),
        py::arg("E"), py::arg("k"), py::arg("ld_logits"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("moe_route_workgroups", &gs::moe_route_workgroups, py::arg("T"));
  m.def("moe_gemm_bf16", &gs::moe_gemm_bf16, py::arg("a"), py::arg("w"), py::arg("sorted_ids"), py::arg("tile_expert"),
        py::arg("out"), py::arg("max_tiles"), py::arg("n_slots"), py::arg("gather_div"), py::arg("N"), py::arg("K"),
        py::arg("lda"), py::arg("ldw"), py::arg("expert_stride"), py::arg("ldc"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("moe_gemm_workgroups", &gs::moe_gemm_workgroups, py::arg("T"), py::arg("k"), py::arg("E"), py::arg("N"));
  m.def("moe_combine_bf16", &gs::moe_combine_bf16, py::arg("y"), py::arg("slot_pos"), py::arg("topk_w"), py::arg("out"),
        py::arg("T"), py::arg("D"), py::arg("k"), py::arg("ld_y"), py::arg("ld_out"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("moe_combine_workgroups", &gs::moe_combine_workgroups, py::arg("T"), py::arg("D"));
  m.attr("MX_FP8") = gs::kMxFp8;
  m.attr("MX_FP4") = gs::kMxFp4;
  m.def("quantize_mx_bf16", &gs::quantize_mx_bf16, py::arg("x"), py::arg("q"), py::arg("scales"), py::arg("T"),
        py::arg("D"), py::arg("ld_x"), py::arg("ld_q"), py::arg("ld_scales"), py::arg("fmt"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("quantize_mx_workgroups", &gs::quantize_mx_workgroups, py::arg("T"), py::arg("D"));
  m.def("gemm_mx_nt", &gs::gemm_mx_nt, py::arg("a"), py::arg("a_scales"), py::arg("w"), py::arg("w_scales"),
        py::arg("c"), py::arg("bias"), py::arg("M"), py::arg("N"), py::arg("K"), py::arg("lda"), py::arg("ld_a_scales"),
        py::arg("ldw"), py::arg("ld_w_scales"), py::arg("ldc"), py::arg("a_fmt"), py::arg("relu"), py::arg("stream"),
        py::arg("cu_budget") = 0, py::call_guard<py::gil_scoped_release>());
  m.def("rope_append_kv8", &gs::rope_append_kv8, py::arg("qkv"), py::arg("cos_sin"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("ctx_lens"),
        py::arg("q_start"), py::arg("q_out"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("max_q_len"),
        py::arg("max_pos"), py::arg("ld_qkv"), py::arg("ld_q_out"), py::arg("ld_table"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("paged_decode_kv8", &gs::paged_decode_kv8, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("ctx_lens"), py::arg("out"),
        py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("ld_q"), py::arg("ld_out"), py::arg("ld_table"),
        py::arg("scale"), py::arg("stream"), py::call_guard<py::gil_scoped_release>());
  m.def("paged_decode_split_kv8", &gs::paged_decode_split_kv8, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("ctx_lens"), py::arg("workspace"),
        py::arg("out"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("kv_splits"), py::arg("ld_q"),
        py::arg("ld_out"), py::arg("ld_table"), py::arg("scale"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("paged_prefill_kv8", &gs::paged_prefill_kv8, py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("ctx_lens"), py::arg("q_start"),
        py::arg("out"), py::arg("S"), py::arg("Hq"), py::arg("Hkv"), py::arg("max_q_len"), py::arg("ld_q"),
        py::arg("ld_out"), py::arg("ld_table"), py::arg("scale"), py::arg("stream"),
        py::call_guard<py::gil_scoped_release>());
  m.def("gemm_mx_workgroups",&gs::gemm_mx_workgroups, py::arg("M"), py::arg("N"), py::arg("K"),
        py::arg("cu_budget") = 0);
  // the launch knobs (GS_KNOBS of api.h): set_<name>(value) for every row, and the whole table at once
  for (int k = 0; k < gs::kNumKnobs; ++k)
    m.def(("set_" + std::string(gs::kKnobs[k].name)).c_str(), [k](int value) { gs::set_knob(gs::Knob(k), value); });
  auto knob_dict = [](bool defaults) {
    py::dict out;
    for (int k = 0; k < gs::kNumKnobs; ++k) out[gs::kKnobs[k].name] = defaults ? gs::kKnobs[k].def : gs::knob(gs::Knob(k));
    return out;
  };
  m.def("knobs", [=]() { return knob_dict(false); });
  m.def("knob_defaults", [=]() { return knob_dict(true); });
  m.def("reset_knobs", &gs::reset_knobs);
  // what gemm_bf16_nt would launch (no GPU needed): the kernels by their demangled names, which the kernel
  // handles carry as dynamic symbols of this module; c_wide_ok = C rows are 16-byte aligned
  m.def("gemm_plan", [](int M, int N, int K, int cu_budget, bool relu, bool bias, bool c_wide_ok, bool workspace) {
    const gs::GemmPlan p = gs::plan_gemm(M, N, K, cu_budget, relu, bias, c_wide_ok && gs::knob(gs::k_wide_epilogue),
                                         workspace);
    py::list launches;
    for (const gs::GemmLaunch& l : p.launches) {
      Dl_info sym{};
      dladdr(l.kernel, &sym);
      char* name = sym.dli_sname ? abi::__cxa_demangle(sym.dli_sname, nullptr, nullptr, nullptr) : nullptr;
      launches.append(py::dict(py::arg("tile") = l.tile, py::arg("kernel") = std::string(name ? name : ""),
                               py::arg("grid") = l.grid, py::arg("block") = l.block, py::arg("xmap") = l.xmap,
                               py::arg("m0") = l.m0, py::arg("m") = l.m));
      std::free(name);
    }
    return py::dict(py::arg("split") = p.split, py::arg("launches") = launches);
  }, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("cu_budget") = 0, py::arg("relu") = false,
        py::arg("bias") = false, py::arg("c_wide_ok") = true, py::arg("workspace") = false);
  m.def("xcd_probe", &gs::xcd_probe, py::arg("out"), py::arg("blocks"), py::arg("stream"));
  m.def("pick_xcd_map", &gs::pick_xcd_map, py::arg("tiles_m"), py::arg("tiles_n"));
  m.def("pick_gemm_tile", &gs::pick_gemm_tile, py::arg("M"), py::arg("N"), py::arg("cu_budget") = 0);
  m.def("gemm_workgroups", &gs::gemm_workgroups, py::arg("M"), py::arg("N"), py::arg("K"), py::arg("cu_budget") = 0,
        py::arg("fp8") = false, py::arg("split_workspace") = false);
  m.def("peer_access_matrix", &gs::peer_access_matrix);
  m.def("peer_copy_gbps", &gs::peer_copy_gbps, py::arg("src"), py::arg("dst"), py::arg("bytes"),
        py::arg("iters") = 10, py::call_guard<py::gil_scoped_release>());
}
