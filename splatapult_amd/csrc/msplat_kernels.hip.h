// msplat_kernels.hip.h -- hand-written CDNA4 (gfx950, wave64) kernels of the splat hot path, in twenty parts.
//
// Replaces (not ports) the reference's GL pipeline:
//   shader/presort_compute.glsl + shader/multi_radixsort*.glsl  -> msplat_sort.hip.h      radix_* / ws_* (cull fused in pass 0)
//   shader/splat_vert.glsl + shader/splat_geom.glsl             -> msplat_project.hip.h   project_kernel
//   GL rasteriser + shader/splat_frag.glsl + ROP blend          -> msplat_binning.hip.h   bin1_* (+ radix_*<MODE_PAIR>)
//                                                                  msplat_composite.hip.h composite_kernel, composite_depth_kernel
//   which splat a pixel shows (no reference part)               -> msplat_ids.hip.h       composite_ids_kernel, mark_ids_kernel
//   what each splat contributes (no reference part)             -> msplat_scores.hip.h    composite_scores_kernel, mark_scores_kernel
//   splats tinted by class at render time (no reference part)   -> msplat_overlay.hip.h   overlay_kernel, overlay_classes_kernel
//   GaussianCloud::ImportPly's per-vertex math, storage order   -> msplat_cloud.hip.h     ingest_kernel, morton / gather / cull boxes
//   splats selected by position, a selection measured (no ref.) -> msplat_select.hip.h    mark_volume_kernel, mark_view_kernel, measure_cloud_kernel
//   splats selected by attribute: values, range, histogram      -> msplat_values.hip.h    cloud_values_kernel, mark_values_kernel, histogram_values_kernel
//   splats selected by neighbourhood: count, nearest (no ref.) -> msplat_neighbours.hip.h neighbour_* (count, sums, starts, scatter, tests, fill, search)
//   the row reduction both measures end with (no ref. part)     -> msplat_rows.hip.h      row_reduce_store, rows_finish_kernel
//   a mask or crop made permanent (no reference part)          -> msplat_compact.hip.h   compact_* (flags, count, offsets, index, gather)
//   splats moved, rotated, scaled in the store (no ref. part)   -> msplat_transform.hip.h transform_kernel
//   splats of a second cloud appended (no reference part)       -> msplat_append.hip.h    append_* (flags, map, gather, convert)
//   splats recoloured and faded in the store (no ref. part)     -> msplat_adjust.hip.h    adjust_kernel
//   GaussianCloud::ExportPly's per-splat math, the way out     -> msplat_download.hip.h  unpack_kernel, egress_kernel
//   shader/point_*.glsl                                         -> msplat_points.hip.h
//   two-pass frame with occlusion feedback (no reference part)  -> msplat_occlusion.hip.h
//   shared constants, FrameParams, cull_key, box_live           -> msplat_common.hip.h
//
// Design notes: everything is HBM/LDS/VALU work -- no MFMA anywhere.
// Compiled with -ffp-contract=off: an FMA happens only where __builtin_fmaf is written.
#pragma once

#include "msplat_common.hip.h"
#include "msplat_sort.hip.h"
#include "msplat_cloud.hip.h"
#include "msplat_rows.hip.h"
#include "msplat_select.hip.h"
#include "msplat_compact.hip.h"
#include "msplat_transform.hip.h"
#include "msplat_append.hip.h"
#include "msplat_adjust.hip.h"
#include "msplat_download.hip.h"
#include "msplat_values.hip.h"
#include "msplat_neighbours.hip.h"
#include "msplat_project.hip.h"
#include "msplat_binning.hip.h"
#include "msplat_composite.hip.h"
#include "msplat_ids.hip.h"
#include "msplat_scores.hip.h"
#include "msplat_overlay.hip.h"
#include "msplat_points.hip.h"
#include "msplat_occlusion.hip.h"
