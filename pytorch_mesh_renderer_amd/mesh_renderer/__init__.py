"""Same export surface as the reference's src/mesh_renderer/__init__.py:1-5."""
from .render import render, tone_mapper, tone_mapper_uint8, to_uint8
from .rasterize import rasterize
from .antialiasing import antialias, antialias_topology
from .sh_lighting import render_sh, sh_shader
from .texturing import (attribute_derivatives, render_textured, render_textured_filtered, texture, texture_filtered,
                        texture_mip_levels)
from . import losses
from . import regularizers
from . import points
from . import preconditioning
from .graphs import capture_step, CapturedStep

__version__ = '0.0.1'
name = 'mesh_renderer'
