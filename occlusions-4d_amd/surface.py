"""The occupancy surface of the dense query grid as a quad mesh, on the device (include/occ4d_surface.h: naive surface nets).

perform_inference(surface=Surface()) adds result['surface'] = dict(vertices (V, 3 + G), faces (F, 4) int32): one vertex per grid
cell the surface crosses -- x, y, z in world coordinates, then all G squashed output columns interpolated onto it --, one quad per
crossed grid edge that four cells share, normals from solid to air.  The mesh is open where the surface leaves the grid.

    res = perform_inference(..., point_sample_mode='grid', surface=Surface())
    write_ply('frame.ply', res['surface']['vertices'], res['surface']['faces'], rgb_columns=(4, 5, 6))

Under refine=GridRefine(...) the mesh is that of the expanded array: with refine.low <= level, a cell whose eight corners all lie
in inactive blocks is never crossed (their densities are copies of the representatives', below `low`), so the surface appears only
where blocks were decoded."""
import numpy as np

from . import ops, products


class Surface(products.LevelProduct):
    """The option object of perform_inference(surface=...) / evaluate_clip(surface=..., meshes=[]).  level: the density at which the
    surface is taken (inside = density >= level, the comparison of the solid split); None = the call's density_threshold.  The
    product: dict(vertices (V, 3 + G) float32, faces (F, 4) int32) (extract); one 8-byte device->host read sizes it."""
    keyword, clip_list = 'surface', ('meshes', 'one mesh')

    def __init__(self, level=None):
        self.level = self._level(level)

    def run(self, grid, level, made):             # (the very floats the query grid was generated from)
        vertices, faces = extract(grid.output, grid.counts, grid.mins, grid.spacings, level)
        return dict(vertices=vertices, faces=faces)

    def __repr__(self):
        return 'Surface(level=%r)' % (self.level,)


def extract(implicit_output, counts, mins, spacings, level, channel=0):
    """The mesh of a dense (N, G) output on the (nx, ny, nz) = `counts` grid whose points ops.grid_points made from `mins` /
    `spacings` (geometry.grid_frame): the surface of column `channel` at `level`, all G columns as vertex attributes.
    -> (vertices (V, 3 + G), faces (F, 4) int32) on the device; one 8-byte device->host read."""
    level = float(level)
    if level != level:
        raise ValueError('surface.extract: level is NaN')
    assert implicit_output.dim() == 2 and 0 <= channel < implicit_output.shape[1], 'channel = %r' % (channel,)
    return ops.surface_nets(implicit_output[:, channel], counts, level, mins, spacings, attrs=implicit_output)


def write_ply(path, vertices, faces, rgb_columns=None):
    """A binary little-endian PLY file of the mesh: float32 x, y, z per vertex, with rgb_columns = three column numbers of
    `vertices` holding colours in [0, 1] also uchar red, green, blue; quads as `list uchar int vertex_indices`."""
    v = np.asarray(vertices.cpu() if hasattr(vertices, 'cpu') else vertices, dtype=np.float32)
    f = np.asarray(faces.cpu() if hasattr(faces, 'cpu') else faces, dtype=np.int32)
    assert v.ndim == 2 and v.shape[1] >= 3 and f.ndim == 2 and f.shape[1] == 4, (v.shape, f.shape)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    if rgb_columns is not None:
        assert len(rgb_columns) == 3
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
    vert = np.zeros(v.shape[0], dtype=fields)
    for a, name in enumerate('xyz'):
        vert[name] = v[:, a]
    if rgb_columns is not None:
        with np.errstate(invalid='ignore'):
            rgb = np.rint(np.clip(np.nan_to_num(v[:, list(rgb_columns)]), 0.0, 1.0) * 255.0).astype(np.uint8)
        for a, name in enumerate(('red', 'green', 'blue')):
            vert[name] = rgb[:, a]
    face = np.zeros(f.shape[0], dtype=[('count', 'u1'), ('index', '<i4', (4,))])
    face['count'] = 4
    face['index'] = f
    header = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % v.shape[0], 'property float x', 'property float y',
              'property float z']
    if rgb_columns is not None:
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    header += ['element face %d' % f.shape[0], 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as out:
        out.write(('\n'.join(header) + '\n').encode('ascii'))
        out.write(vert.tobytes())
        out.write(face.tobytes())
