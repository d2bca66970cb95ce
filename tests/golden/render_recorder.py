"""A recording stand-in for the module the reference's render() imports as `mate.assets.pygletrendering`: no window, no GL.  It offers the names
environment.py:986-1180 uses (Viewer, Transform, Compound, Image, make_polygon, make_circle, and on the geoms: attrs, color.vec4, set_color, add_attr,
set_linewidth, gs) and, at Viewer.render(), walks the static geoms and then the one-time geoms in order and appends one record per primitive to
`Viewer.recorded`: (kind, world-space vertices [n, 2] f64 after every enclosing transform, the RGBA in force, the line width).  A geom's attributes take
effect last-added first, as the reference's Geom.render enables them, so a Compound's transform encloses its parts and a part's own colour replaces the
Compound's.  Written for tests/golden/make_render_golden.py; the tests never import it.
"""
import math

import numpy as np

RECORDS = []      # every Viewer appends here too: the maker reads the last frame from the viewer itself


class Color:
    def __init__(self, vec4):
        self.vec4 = vec4


class LineWidth:
    def __init__(self, stroke):
        self.stroke = stroke


class Transform:
    def __init__(self, translation=(0.0, 0.0), rotation=0.0, scale=(1, 1)):
        self.set_translation(*translation)
        self.set_rotation(rotation)
        self.set_scale(*scale)

    def set_translation(self, newx, newy):
        self.translation = (float(newx), float(newy))

    def set_rotation(self, new):
        self.rotation = float(new)

    def set_scale(self, newx, newy):
        self.scale = (float(newx), float(newy))

    def matrix(self):
        cs, sn = math.cos(self.rotation), math.sin(self.rotation)
        sx, sy = self.scale
        return np.array([[cs * sx, -sn * sy, self.translation[0]], [sn * sx, cs * sy, self.translation[1]], [0.0, 0.0, 1.0]])


class _Pen:
    """What GL would hold while the list is drawn: the matrix stack's top, the colour, the line width."""

    def __init__(self):
        self.matrix, self.rgba, self.width, self.out = np.eye(3), (0.0, 0.0, 0.0, 1.0), 1.0, []

    def emit(self, kind, vertices):
        v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
        world = v @ self.matrix[:2, :2].T + self.matrix[:2, 2]
        self.out.append({'kind': kind, 'v': world, 'rgba': tuple(float(x) for x in self.rgba), 'width': float(self.width)})


class Geom:
    def __init__(self):
        self.color = Color((0, 0, 0, 1.0))
        self.attrs = [self.color]

    def add_attr(self, attr):
        self.attrs.append(attr)

    def set_color(self, r, g, b, a=1.0):
        self.color.vec4 = (r, g, b, a)

    def draw(self, pen):
        saved = pen.matrix
        for attr in reversed(self.attrs):
            if isinstance(attr, Transform):
                pen.matrix = pen.matrix @ attr.matrix()
            elif isinstance(attr, Color):
                pen.rgba = tuple(attr.vec4)
            elif isinstance(attr, LineWidth):
                pen.width = attr.stroke
        self.draw1(pen)
        pen.matrix = saved

    def draw1(self, pen):
        raise NotImplementedError


class FilledPolygon(Geom):
    def __init__(self, v):
        super().__init__()
        self.v = v

    def draw1(self, pen):
        pen.emit('polygon', self.v)


class PolyLine(Geom):
    def __init__(self, v, close):
        super().__init__()
        assert close, 'the display list holds closed polylines only'
        self.v, self.close = v, close
        self.linewidth = LineWidth(1)
        self.add_attr(self.linewidth)

    def set_linewidth(self, x):
        self.linewidth.stroke = x

    def draw1(self, pen):
        pen.emit('polyline', self.v)


class Image(Geom):
    def __init__(self, fname, width, height):
        super().__init__()
        self.fname, self.width, self.height = str(fname), width, height

    def draw1(self, pen):
        w, h = self.width, self.height
        pen.emit('image', [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)])


class Compound(Geom):
    def __init__(self, gs):
        super().__init__()
        self.gs = gs
        for g in self.gs:
            g.attrs = [a for a in g.attrs if not isinstance(a, Color)]

    def draw1(self, pen):
        for g in self.gs:
            g.draw(pen)


def make_circle(radius=10, res=30, filled=True):
    points = [(math.cos(2 * math.pi * i / res) * radius, math.sin(2 * math.pi * i / res) * radius) for i in range(res)]
    return FilledPolygon(points) if filled else PolyLine(points, True)


def make_polygon(v, filled=True):
    return FilledPolygon(v) if filled else PolyLine(v, True)


class Viewer:
    def __init__(self, width, height, display=None):
        self.width, self.height = width, height
        self.geoms, self.onetime_geoms, self.recorded, self.bounds, self.isopen = [], [], [], None, True

    def set_bounds(self, left, right, bottom, top):
        self.bounds = (left, right, bottom, top)

    def add_geom(self, geom):
        self.geoms.append(geom)

    def add_onetime(self, geom):
        self.onetime_geoms.append(geom)

    def render(self, return_rgb_array=False):
        pen = _Pen()
        for geom in self.geoms + self.onetime_geoms:
            geom.draw(pen)
        self.recorded = pen.out
        RECORDS.append(pen.out)
        self.onetime_geoms = []
        return np.zeros((self.height, self.width, 3), dtype=np.uint8) if return_rgb_array else self.isopen

    def close(self):
        self.isopen = False
