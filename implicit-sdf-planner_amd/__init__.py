"""implicit-sdf-planner_amd — MI355X-native collision cost/gradient engine (one hot path of Implicit-SDF-Planner).

Host-side Python mirror of the C-ABI in include/isdf_accel.h.  The compute lives in csrc/ (hand-written HIP for
gfx950, built into lib/libisdf_accel.so); this package only marshals arrays.  Import name: ``isdf_amd``
(the directory name contains a hyphen; __graft_entry__.load_package() registers the alias).
"""
from . import capi, synth, parallel, fixtures, csg  # noqa: F401
from .engine import Engine, IsdfError, lbfgs_minimize, write_obj, traj_limits_host, traj_sample_host, traj_retime_host, traj_scale_host, traj_realloc_host, traj_minco_host, frontend_field_host, frontend_field_repair_host, frontend_field_reopen_host, frontend_field_shift_host, traj_check_fold_host, shift_geometry_host, shift_grid_host, shift_bands_host  # noqa: F401
