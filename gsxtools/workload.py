"""The pod workload: ``samples/workload/main.py``, the file the sample image ships, loaded from there.

The harness (``python -m gsxtools.workload``, the isolation bench, ``ProcessRuntime`` pods) runs the very code the
container runs; ``libgsx_kernels.so`` is found in the repository's build tree (the image builds its own copy).
"""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

_MAIN = Path(__file__).resolve().parents[1] / "samples" / "workload" / "main.py"
_spec = importlib.util.spec_from_file_location("gsx_sample_workload", _MAIN)
_mod = importlib.util.module_from_spec(_spec)
sys.modules.setdefault("gsx_sample_workload", _mod)
_spec.loader.exec_module(_mod)

run = _mod.run
main = _mod.main
build_parser = _mod.build_parser
parse_mask = _mod.parse_mask
kernels_lib_path = _mod.kernels_lib_path
matrix_bytes = _mod.matrix_bytes
default_weights_bytes = _mod.default_weights_bytes
ring_layers = _mod.ring_layers
kv_layer_bytes = _mod.kv_layer_bytes
kv_pages = _mod.kv_pages
default_kv_bytes = _mod.default_kv_bytes
kv_ring_layers = _mod.kv_ring_layers
add_attn_arguments = _mod.add_attn_arguments
server_layer_weight_bytes = _mod.server_layer_weight_bytes
server_window = _mod.server_window
default_ffn = _mod.default_ffn
layer_weight_bytes = _mod.layer_weight_bytes
prefill_refusal = _mod.prefill_refusal
prefill_visible_pairs = _mod.prefill_visible_pairs
add_generate_arguments = _mod.add_generate_arguments
generate_refusal = _mod.generate_refusal
generate_step_bytes = _mod.generate_step_bytes
add_moe_arguments = _mod.add_moe_arguments
moe_refusal = _mod.moe_refusal
moe_active = _mod.moe_active
moe_expert_bytes = _mod.moe_expert_bytes
moe_layer_weight_bytes = _mod.moe_layer_weight_bytes
moe_layer_read_bytes = _mod.moe_layer_read_bytes
BatchRangeParser = _mod._Parser

if __name__ == "__main__":
    sys.exit(main())
