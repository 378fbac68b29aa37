"""Tensor-level wrappers over the C ABI (include/tavsr.h), one submodule per kernel family, plus ``streams``: which queue a launch
goes to and what orders the queues (fork / join scopes, weight gradients beside the backward chain, the race amplifier).
The wrappers do no autograd and no torch arithmetic: torch allocates buffers on the caching allocator and names the current
stream.  Every function raises ``TavsrError`` on a CPU tensor or a failed call - there is no fallback.

``from tavsr import ops`` and ``ops.<name>`` reach every wrapper.  The route switches and limits of all families are defined
HERE, once, and the submodules read them at call time as ``ops.<NAME>``: an in-process assignment (``ops.LAYER_C = False``; tests,
bench.py, scripts/) takes effect at the next call.  No submodule binds one of them itself (tests/test_host_api.py).
"""
from __future__ import annotations

import os
from typing import Optional

# ---------------------------------------------------------------------------------------------- matmul
PROFILE: Optional[GemmProfile] = None      # a ``GemmProfile``: per-launch timing of tavsr_gemm (bench.py's roofline leg); None on the product path

# ---------------------------------------------------------------------------------------------- streams
# Weight gradients on the owner's side queue, un-joined until the end of the autograd pass (``streams.wgrad_beside``: the comment
# above ``streams._WGRAD_OPEN`` has the reasoning and the conditions).  TAVSR_WGRAD_BESIDE=0: on the backward chain's own queue.
WGRAD_BESIDE = os.environ.get("TAVSR_WGRAD_BESIDE", "1") != "0"
WGRAD_SLOT = int(os.environ.get("TAVSR_WGRAD_SLOT", "0"))

# ---------------------------------------------------------------------------------------------- norm
LN_BWD_DROP = True      # masked gradient copy from the LayerNorm backward (tests flip it in-process to compare with the dropout launch)

# ---------------------------------------------------------------------------------------------- attention
# Fused attention core (csrc/attn_fused.hip): scores, rel_shift, mask, softmax, dropout and the context product in one
# launch per direction.  TAVSR_ATTN_FUSED=0 keeps the GEMM + softmax chain (A/B switch; also the path for head sizes != 64).
ATTN_FUSED = True

# Additive attention (csrc/fastattn.hip): what tavsr_fastattn_ok takes; FastSelfAttention's constructor refuses the rest in these words
# (the range itself: ops.fastattn_ok in ops/fastattn.py and fa_shape_ok in csrc/fastattn.hip - the three change together)
FASTATTN_LIMIT = "1 <= attention_heads <= 8, size <= 512, size / attention_heads a multiple of 4"

# ---------------------------------------------------------------------------------------------- blocks
# Streaming feed-forward block (csrc/ffn2.hip, round 3): LayerNorm prologue + both GEMMs in one launch whose weights stream
# through per-wave LDS-DMA rings, + a finishing launch that can also emit the LayerNorms the consumers of y start with.
# Shapes it does not take keep the LayerNorm + GEMM + GEMM launches; tests flip these two in-process to compare the routes.
FFN2 = True
FFN2_BWD = True      # the dgrad pair of the block as the streaming kernel too
FFN2_BWD_LN = os.environ.get("TAVSR_FFN2_BWD_LN", "1") != "0"      # the block's LayerNorm backward sums dn's partials itself (no finishing launch); flipped in tests/test_gpu_switches.py

# One Branchformer layer forward as ONE C call (csrc/layer.hip): the same launches, sequenced in C.  For un-captured loops
# (the host is what limits an eager step); a captured step replays the same kernels either way.  TAVSR_LAYER_C=0: Python sequencing.
LAYER_C = os.environ.get("TAVSR_LAYER_C", "1") != "0"
LAYER_C_EAGER_ONLY = os.environ.get("TAVSR_LAYER_C", "1") != "capture"     # TAVSR_LAYER_C=capture: also while a hipGraph is being captured
BLOCKS_C = os.environ.get("TAVSR_BLOCKS_C", "1") != "0"      # block-level C entry points (tavsr_conv2d_subsample_*, tavsr_cgmlp_fwd) instead of launch-by-launch sequencing

CSGU_FUSED = True
CSGU_STATS_IN_GEMM = True
CGMLP_ACT_BWD_FUSED = True   # gelu' in the CSGU's two backward kernels

MERGE_ROWS = True      # the row-parallel learned_ave merge launches (D = 256; tests flip it in-process to compare the routes)
MERGE_PROJ = os.environ.get("TAVSR_MERGE_PROJ", "1") == "1"      # A/B switch: merge + merge_proj + residual as one launch
MERGE_ROWDOT = True      # the fused tail reads the merge's row dots from the producers' GEMM epilogues (flipped in tests/test_gpu_switches.py)

# ---------------------------------------------------------------------------------------------- vision
# Conv3d stem as an implicit GEMM (tavsr_gemm_desc.conv_mode 4 / 5): no 6 GB patch matrix.  TAVSR_STEM_IMPLICIT=0 returns to
# im2col_stem + plain GEMMs (A/B switch; also the route for shapes the gather loader does not take).
STEM_IMPLICIT = True
# Default stem route: zero-padded clips + taps laid out 35 x 8, fetched with the GEMM's ordinary 16-byte LDS-DMA (conv_mode 6 / 7).
# TAVSR_STEM_PAD16=0: the 4-byte gather route (conv_mode 4 / 5, no padded copy of the clips).
STEM_PAD16 = True

# Padding taps of the stride-1 3x3 / pad 1 convolutions (tavsr_gemm_desc.conv_posmajor): forward and data gradient walk their
# rows position-major and skip the K-steps of the taps that are padding for a whole tile (bit-identical results); the weight
# gradient walks the pixels of a K slice position-major and skips the steps where its tile's tap is padding.  Forward and data
# gradient: maps of at most CONV_TAPSKIP_MAXPOS positions (trunk layers 2 - 4: 11x11, 6x6, 3x3; the 11x11 map lost under the
# unbalanced tile order of round 6 and gains 10 % of its launches under CONV_TILEORDER; on layer 1's 22x22 map 6 % of the taps
# are padding).  TAVSR_CONV_TAPSKIP=0: the launches without the flag (A/B switch).
CONV_TAPSKIP = os.environ.get("TAVSR_CONV_TAPSKIP", "1") != "0"
CONV_TAPSKIP_MAXPOS = int(os.environ.get("TAVSR_CONV_TAPSKIP_MAXPOS", "121"))
# Tile order of the position-major forward / data gradient launches: tiles sorted by tap count and dealt evenly to the XCDs
# (csrc/gemm_conv.hip, struct TileOrder; bit-identical results).  TAVSR_CONV_TILEORDER=0: one contiguous range of tiles per XCD, as
# before (A/B switch; bit 1 of conv_posmajor).
CONV_TILEORDER = os.environ.get("TAVSR_CONV_TILEORDER", "1") != "0"
# The weight gradient has a gate of its own: its position-major walk costs bookkeeping per K-step that the forward does not
# pay, so a map can gain in one direction and lose in the other: the 11x11 map's weight gradient is 4 % SLOWER with the skip
# (profiles/r08_notes.md has the per-shape rows behind both gates) and stays outside.
CONV_TAPSKIP_MAXPOS_DW = int(os.environ.get("TAVSR_CONV_TAPSKIP_MAXPOS_DW", "36"))
# K slices of two lengths for the position-major weight gradient where equal slices leave block slots empty (csrc/gemm_conv.hip,
# plan_conv: trunk layer 3 at 3200 frames, 32 slices instead of 24; another summation order).  TAVSR_CONV_DW_UNEVEN=0: equal
# slices, as before (A/B switch; bit 2 of conv_posmajor).
CONV_DW_UNEVEN = os.environ.get("TAVSR_CONV_DW_UNEVEN", "1") != "0"

# The stride-2 3x3 / pad 1 convolutions that open trunk layers 3 and 4 (11 -> 6 and 6 -> 3: 0.79 of the taps inside the image;
# bit 3 of conv_posmajor, honoured up to 6x6 output positions, so layer 2's 22 -> 11 keeps its launch): forward, bit-identical,
# and weight gradient, another summation order, each with its own switch (TAVSR_CONV_TAPSKIP_STRIDE2 / _STRIDE2_DW = 0 / 1).
# The forward gains 21 % of its two launches and is on; the weight gradient gained 7 % on one launch and lost 4 % on the other,
# inside the call's noise in sum, and ships off (profiles/r08_notes.md).
CONV_TAPSKIP_STRIDE2 = os.environ.get("TAVSR_CONV_TAPSKIP_STRIDE2", "1") != "0"
CONV_TAPSKIP_STRIDE2_DW = os.environ.get("TAVSR_CONV_TAPSKIP_STRIDE2_DW", "0") != "0"
CONV_TAPSKIP_STRIDE2_MAXPOS = 36
# Forward and data gradient of the trunk's 3x3 / 1x1 convolutions on bf16 MFMA over three-way split fp32 operands
# (bit 4 of tavsr_gemm_desc.conv_posmajor, csrc/gemm_glds.h "split operands"): six bf16 products per fp32 product, fp32-level error, another
# rounding than the fp32 MFMA's.  The weights are split once per step (ops.conv_wsplit), the activations in the kernel.
# TAVSR_CONV_X6=0: the fp32 launches, bit-identical to what they were (A/B switch).
CONV_X6 = os.environ.get("TAVSR_CONV_X6", "1") != "0"
# The same for the weight gradient of these convolutions (bit 5 of conv_posmajor; csrc/gemm_conv.hip, conv_x6_dw): both operands are
# activations, so both are split in the kernel, from the fp32 images the fp32 launch stages - same tiles, K split and orders.  A
# switch of its own: CONV_X6 does not reach the weight gradient.  The bias gradient of the launch stays fp32, bit for bit.
# TAVSR_CONV_X6_DW=0: the fp32 launches, bit-identical to what they were (A/B switch).
CONV_X6_DW = os.environ.get("TAVSR_CONV_X6_DW", "1") != "0"

# ---------------------------------------------------------------------------------------------- losses
CTC_ALIGN_CHUNK = 16      # frames of emissions the alignment kernel gathers into LDS at a time (kAlignChunk, csrc/ctc.hip)
# Validation CER / WER on the device (csrc/editdist.hip; ErrorCalculator in models/espnet_model.py picks the route per call).
# TAVSR_DEVICE_ERROR_RATES=0: the host route, ids copied to the host and a Python edit distance (A/B switch; the same integers).
DEVICE_ERROR_RATES = os.environ.get("TAVSR_DEVICE_ERROR_RATES", "1") != "0"

# ---------------------------------------------------------------------------------------------- data
RESAMPLE_ROLLOFF, RESAMPLE_ZEROS, RESAMPLE_BETA = 0.9475937167399596, 64, 14.769656459379492      # "kaiser_best" filter constants

# ---------------------------------------------------------------------------------------------- search
ROWLIN = True
ROWLIN_KSPLIT = 4      # K slices of the 2048 -> d projection of a one-token feed-forward block; 1: one block per tile (<= 16 rows only)
TREE_ROWS_MAX_KEYS = 1024      # keys per row that tavsr_tree_attn_rows takes (its per-wave LDS arrays; include/tavsr.h)
RNNT_SEARCH_KINDS = {"alsd": 0, "tsd": 1}
RNNT_SEARCH_LIMIT = ("1 <= beam <= 64, beam < vocabulary, at least one frame, u_max >= 0, 1 <= max_sym_exp <= 8, the trie of an "
                     "utterance within 2^30 words")

# ---------------------------------------------------------------------------------------------- rnnt
RNNT_WS_FLOATS = 1 << 24      # bound of a chunk's logits (64 MB): the default chunk is the number of rows that fit it

# The families, after the switches: each submodule does ``from .. import ops`` and finds the names above already bound.
from .base import *  # noqa: E402,F401,F403
from .rng import *  # noqa: E402,F401,F403
from .streams import *  # noqa: E402,F401,F403
from .data import *  # noqa: E402,F401,F403
from .blocks import *  # noqa: E402,F401,F403
from .matmul import *  # noqa: E402,F401,F403
from .norm import *  # noqa: E402,F401,F403
from .attention import *  # noqa: E402,F401,F403
from .fastattn import *  # noqa: E402,F401,F403
from .vision import *  # noqa: E402,F401,F403
from .losses import *  # noqa: E402,F401,F403
from .search import *  # noqa: E402,F401,F403
from .rnnt import *  # noqa: E402,F401,F403
