// kernels.hpp — every device kernel of the library (gfx950), one file per kernel family.  Host code, the run-time compiled traced
// models and the tools under tools/ubench include this file; the files below hold no host-only header and are found next to it.
// Every one of them is listed in fib_tf_amd/_lib.py DEPS.
#pragma once
#include "models.hpp"

namespace fib {
FIB_TAG_BEGIN
#include "stencil.hpp"          // Geo, PtrTab, PhaseTab; stencil9, lap9, add_phase, PhaseCoef; xcd_tile, ZeroPadOf, TensorOf, lap9_tensor, TwoPass
#include "tick_kernel.inc"      // tick_kernel: flat tiles, any K
#include "strip_mt.hpp"         // several ticks in one launch: the protocol, MtArgs, the MT_* constants
#include "strip_kernel.inc"     // FIB_STAMP; strip_body, strip_kernel, strip_mt_kernel
#include "rows_kernel.inc"      // lane_west / lane_east, rows_body, rows_kernel
#include "pointwise.inc"        // pointwise_kernel, unit_op_kernel, phase_prep_kernel, tensor_prep_kernel, unit_tensor_kernel, pace_kernel, court_inter_kernel
#include "record_kernels.inc"   // observe_kernel, electrode_kernel, electrode_combine_kernel, tip_kernel, frame_kernel, stats_kernel, stats_combine_kernel, spectrum_sample_kernel, spectrum_fold_kernel, spectrum_peak_kernel, beat_kernel, beat_summary_kernel, lead_kernel, lead_combine_kernel, pmap_source_kernel, pmap_conv_kernel, pmap_summary_kernel, wave_label_kernel, wave_merge_kernel, wave_root_kernel, wave_reduce_kernel, wave_link_kernel, wave_link_pack_kernel; copy_kernel; stim_kernel; sense_kernel, trigger_kernel, stim_gated_kernel; lesion_apply_kernel, lesion_prep_kernel
FIB_TAG_END
}  // namespace fib
