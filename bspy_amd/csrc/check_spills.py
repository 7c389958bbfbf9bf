"""Build-time guard: the kernels that read LDS through inline asm (eval_stream, jac_stream, eval_rowrot, jac_rowrot)
must not use scratch: a spilled asm destination would be stored before its data arrived.  The fit kernels (fit_sweep's
register windows, fit_transpose, fit_residual) are held to the same: a window in scratch would double their traffic.
So are roots_flag and roots_isolate: their de Casteljau triangles and the interval stack are register arrays by design,
and roots2_flag, roots2_isolate and roots2_merge: the three coefficient arrays of a bivariate walk are register arrays,
and roots3_flag, roots3_isolate and roots3_merge: a wave holds a trivariate cell with one coefficient per lane, six doubles,
and band_absmax, band_absmax_line and band_absmax_fold: the row maxima and the window of band_absmax are register arrays,
and project_seed and project_newton: the point, the iteration's state and one component's de Casteljau arrays are registers,
and contour_flag and contour_march: the box's coefficients, its halves and the de Casteljau triangles of a leaf are register arrays,
and iso_flag, iso_walk, iso_leaf and iso_vertex: a wave holds a cell with one coefficient per lane; a leaf's or an edge's cell is a register array,
and mesh_bound, mesh_count, mesh_emit and mesh_vertex: a cell's window of one component and its difference sums are register arrays,
and ray_boxes, ray_search (ray_count and ray_emit), ray_isolate and ray_reduce: the frame of a ray and the coefficients it forms are registers,
and ssx_search (ssx_count and ssx_emit), ssx_isolate and ssx_merge: a segment's points, their box and the walk's six doubles a lane are registers,
and scatter_key, scatter_gram, scatter_cell, scatter_fold and scatter_residual: a slab row, a point's basis values and a tree's inputs are registers,
and scatter_reweight, scatter_band, scatter_panel, scatter_trail, scatter_forward and scatter_backward: a panel's column is a register array.
Usage: python check_spills.py <resource-usage log>"""
import re
import sys

log = open(sys.argv[1]).read()
bad = []
for m in re.finditer(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", log, re.S):
    name, scratch = m.group(1), int(m.group(2))
    if "eval_slab2IdLi6" in name:       # fp64, order 6: plain C++ instantiation, no asm LDS reads (bsk_slab.hpp)
        continue
    if (any(k in name for k in ("eval_stream", "jac_stream", "eval_rowrot", "jac_rowrot", "curv_rowrot", "eval_uni", "jac_uni", "curv_uni", "eval_slab2", "eval_rec32", "fit_sweep", "fit_transpose", "fit_residual", "roots_flag", "roots_isolate", "roots2_flag", "roots2_isolate", "roots2_merge", "roots3_flag", "roots3_isolate", "roots3_merge", "band_absmax", "project_seed", "project_newton", "contour_flag", "contour_march", "iso_flag", "iso_walk", "iso_leaf", "iso_vertex", "mesh_bound", "mesh_count", "mesh_emit", "mesh_vertex", "ray_boxes", "ray_search", "ray_isolate", "ray_reduce", "ssx_search", "ssx_isolate", "ssx_merge", "scatter_key", "scatter_gram", "scatter_cell", "scatter_fold", "scatter_residual", "scatter_reweight", "scatter_band", "scatter_panel", "scatter_trail", "scatter_forward", "scatter_backward"))) and scratch:
        bad.append((name, scratch))
if bad:
    for name, scratch in bad:
        print(f"SPILL in asm-LDS kernel {name}: {scratch} bytes/lane", file=sys.stderr)
    sys.exit(1)
print("no scratch in asm-LDS kernels")
