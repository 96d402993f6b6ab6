"""occlusions-4d hot path (point-transformer encode + cross-attention implicit
decode of 4D query points) as hand-written HIP for MI355X / gfx950.

Host side mirrors the reference's ``model/`` + ``eval/inference.py`` interface
(same module / class names, constructor kwargs, parameter names and forward
signatures); every forward runs on the C-ABI library
``libocc4d.so`` (include/occ4d.h) and raises if it is missing -- there is no CPU
fallback.  ``configs`` is pure host code (named configurations, synthetic inputs).
"""
from . import configs  # noqa: F401
from . import _lib  # noqa: F401
from . import kernels  # noqa: F401   (`with occlusions4d_amd.kernels(precision='bf16x6'):` -- per-thread kernel selection)
from . import ops  # noqa: F401
from . import autograd  # noqa: F401
from . import products  # noqa: F401   (what the grid options of perform_inference share: Grid, GridProduct, columns)
from . import surface  # noqa: F401   (the occupancy surface as a quad mesh: Surface, extract, write_ply)
from . import point_transformer_layer, modules, model, geometry, implicit, inference, distributed, training  # noqa: F401
from . import evaluation  # noqa: F401
from . import occlusion  # noqa: F401   (valo ids, live occlusion fractions, track id: the id histogram)
from . import frontend  # noqa: F401   (frames -> clouds on the device: greater_clip / carla_clip)
from . import projection  # noqa: F401   (clouds -> camera views: projection, z-buffer, visibility codes; the decoded field ray-cast: FieldViews; the labelled objects as depth layers: ObjectLayers, object_layers, amodal_mask, visible_mask, occlusion_rate, occlusion_pairs)
from . import components  # noqa: F401   (connected components of the decoded occupancy: Components, label, boxes_and_centroids; linked across frames: Tracker, tracks; oriented boxes: Boxes, yaw_directions, oriented_boxes)
from . import distance  # noqa: F401   (the distance transform of the decoded occupancy: Clearance, transform, metric, signed, expand_labels)
from . import geodesic  # noqa: F401   (shortest free-space paths over the clearance: Route, solve, grid_index, metric, paths_to_world; pulled straight into waypoints: straight, pull, polyline_length)
from . import watershed  # noqa: F401   (touching objects split at their necks: Segments, split)
from . import sight  # noqa: F401   (line of sight through the decoded occupancy: Sight, look, grid_origin, codes, by_label; the next best view: NextView, plan, cells_to_world)
from . import sweep  # noqa: F401   (the decoded field scanned by a virtual lidar: FieldSweep, cast, lidar_directions, directions_to, poses, march_range, rows_of, residual)
from . import evidence  # noqa: F401   (measured returns carved into the query grid: Evidence, carve, classify, observe, by_label, rates and the six codes)
from . import cpu_twin  # noqa: F401   (explicit opt-in only: pk.cpu_twin.enable(); never a fallback)

__all__ = ['configs', 'kernels', 'ops', 'point_transformer_layer', 'modules', 'model', 'geometry', 'implicit',
           'inference', 'distributed', 'autograd', 'training', 'evaluation', 'occlusion', 'frontend', 'projection', 'surface',
           'components', 'distance', 'geodesic', 'watershed', 'sight', 'sweep', 'evidence']
