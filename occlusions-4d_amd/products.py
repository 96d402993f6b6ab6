"""The grid products of perform_inference: what its options surface, views, components, tracker, clearance, segments, boxes (components.Boxes), layers (projection.ObjectLayers), sweep (sweep.FieldSweep), evidence (evidence.Evidence), sight,
next_view and route have in common.
Each of them turns the squashed (N, G) output of a point_sample_mode='grid' call into more device tensors, which come home under the
call's one host wait.  An option class derives from GridProduct and says which keyword it answers to, what it needs and how it
runs; perform_inference and evaluate_clip walk the options they are given and know nothing else about them."""


class Grid:
    """The query grid of one perform_inference call: counts (nx, ny, nz), mins, spacings = `frame` (geometry.grid_frame, evaluated
    once per call), the call's density_threshold, predict_segmentation, semantic_classes and device; after the decode also `output`,
    the squashed -- in track_mode 'all' merged, under `refine` expanded -- (N, G) device tensor, and `points`, the (N, 3) device view
    of the call's own query points."""
    output = points = None

    def __init__(self, frame, density_threshold, predict_segmentation, semantic_classes, device):
        self.counts, self.mins, self.spacings = tuple(frame[0]), frame[1], frame[2]
        self.density_threshold, self.predict_segmentation = density_threshold, predict_segmentation
        self.semantic_classes, self.device = semantic_classes, device


class GridProduct:
    """The base of the option classes.  keyword: the perform_inference / evaluate_clip keyword, and the key of the product's dict in
    the result; into: the keyword of the product whose dict this one's tensors join instead; clip_list = (evaluate_clip's list
    keyword, what a frame appends to it); needs = (the keyword that has to be given too, the ValueError's text); reads_grid: whether
    the product itself needs point_sample_mode 'grid'."""
    keyword = into = clip_list = needs = None
    reads_grid = True

    @classmethod
    def check(cls, option, given, point_sample_mode='grid'):
        """ValueError unless `option` is one of these, the call samples the grid and the product it builds on is among the keywords
        `given`."""
        if not isinstance(option, cls):
            raise ValueError('%s must be a %s.%s or None, got %r' % (cls.keyword, cls.__module__.rpartition('.')[2], cls.__name__, option))
        if cls.reads_grid and point_sample_mode != 'grid':
            raise ValueError("%s needs point_sample_mode 'grid', got %r" % (cls.keyword, point_sample_mode))
        if cls.needs is not None and cls.needs[0] not in given:
            raise ValueError(cls.needs[1])

    def prepare(self, grid):
        """Host work before the encode: whatever can be checked (ValueError) or computed from the Grid alone -> handed to run()."""
        return None

    def run(self, grid, prepared, made):
        """After the decode -> an ordered dict name -> device tensor.  made: {keyword: such a dict} of the products that ran before."""
        raise NotImplementedError


class LevelProduct(GridProduct):
    """A product of the set density >= level (or of its boundary); level None = the call's density_threshold."""

    @classmethod
    def _level(cls, level):
        if level is not None:
            level = float(level)
            if level != level:
                raise ValueError('%s: level is NaN' % cls.__name__)
        return level

    def resolve(self, density_threshold):
        return self._level(density_threshold if self.level is None else self.level)

    def prepare(self, grid):
        return self.resolve(grid.density_threshold)


def columns(out, channel, select):
    """The values column `channel` of a dense (N, G) output and, with select = (column, threshold), its mask column -> (values,
    mask or None, mask_level)."""
    assert out.dim() == 2 and 0 <= channel < out.shape[1], 'channel = %r' % (channel,)
    mask, mask_level = None, 0.0
    if select is not None:
        column, mask_level = int(select[0]), float(select[1])
        assert 0 <= column < out.shape[1], 'select column = %r' % (column,)
        mask = out[:, column]
    return out[:, channel], mask, mask_level


def prepare(slots, grid, point_sample_mode):
    """perform_inference's side: slots = (class, option or None) in its order.  Checks every given option (ValueError) and prepares
    it -> [(option, prepared)]."""
    given = [cls.keyword for cls, option in slots if option is not None]
    plan = []
    for cls, option in slots:
        if option is not None:
            cls.check(option, given, point_sample_mode)
            plan.append((option, option.prepare(grid)))
    return plan


def check_clip(slots):
    """evaluate_clip's side: slots = (class, option or None, the caller's list or None) in its order.  Checks every given option and
    its list (ValueError) -> [(option, list)]."""
    given = [cls.keyword for cls, option, _ in slots if option is not None]
    chosen = []
    for cls, option, into in slots:
        if option is not None:
            cls.check(option, given)
            if cls.clip_list is not None and not isinstance(into, list):
                raise ValueError('evaluate_clip(%s=...) needs %s=<a list>: %s per output frame is appended to it'
                                 % (cls.keyword, cls.clip_list[0], cls.clip_list[1]))
            chosen.append((option, into))
    return chosen
