"""Numeric knobs of the prediction path.

Values mirror the reference's module constants (robotpose/constants.py:11-32,60-91)
so that crops, lookup grids and render colours come out identical.
"""
import numpy as np

MAX_LINKS = 7                     # constants.py:11
NUM_RENDER_LINKS = 6              # link_6_t is never rendered (render_utils.py:31-32)

# Crop search (constants.py:19-23)
CROP_RENDER_WEIGHTING = (6, 3, 3, 0, 1, 0)
CROP_VARYING = 'SLUB'
CROP_MAX_PER_JOINT = 50
CROP_SEC_ALLOTTED_APPROX = 20
CROP_PADDING = 10

# Lookup (constants.py:28-32)
GPU_MEMORY_ALLOWED_FOR_LOOKUP = 0.1
LOOKUP_MAX_DIV_PER_LINK = 200
LOOKUP_JOINTS = 'SLU'
LOOKUP_NUM_RENDERED = 6

DEFAULT_CAMERA_POSE = [0, -1.5, .75, 0, 0, 0]      # constants.py:60
RENDERER_FALLBACK_CAMERA_POSE = [0.04, -1.425, 0.75, 0, -0.02, -0.05]   # render.py:49

JOINT_LETTERS = 'SLURBT'          # utils.py:54

# pyrender.IntrinsicsCamera defaults used by the reference (projection.py:161-169)
ZNEAR = 0.05
ZFAR = 100.0


def render_colors(num: int = MAX_LINKS):
    """Flat segmentation colours, channel 0 unique per link (constants.py:65-91).

    b = linspace(0,255,num) truncated to int, g = 0, r = |255 - 2b|.
    """
    b = np.linspace(0, 255, num).astype(int)
    return [[int(bi), 0, int(abs(255 - 2 * bi))] for bi in b]


DEFAULT_RENDER_COLORS = render_colors(MAX_LINKS)
# channel-0 value per rendered link id; 255 marks background in the engine's id image
LINK_BLUE = np.array([c[0] for c in DEFAULT_RENDER_COLORS], dtype=np.uint8)
BACKGROUND_ID = 255
VIDEO_FPS = 15      # default preview video frames per second (constants.py:58)
JSON_LINK_FILE = r"\\marvin\ROPE\joint_states.json"      # where the controller drops its joint state (constants.py:16)

# Verifier (constants.py:49-53,59); VERIFIER_SELECTED_GAMMA belongs to the click-through GUI, which is not here
VERIFIER_ALPHA = .7               # weight of the photograph in an overlay; the render takes the rest
VERIFIER_SCALER = 1.5             # overlay size over the thumbnail's: the frame is shown at VERIFIER_SCALER / THUMBNAIL_DS_FACTOR
VERIFIER_ROWS = 4                 # overlays per contact sheet: rows x columns
VERIFIER_COLUMNS = 4
THUMBNAIL_DS_FACTOR = 6           # a dataset's preview images are the frames shrunk by this factor (building.py:183-185)

# Photo-like synthetic frames (simulation/shading.py: draw_params, make_backgrounds).  These ranges are this project's choice: the
# reference has no such stage, and nothing here was fitted to a real camera.
SHADE_AMBIENT = .12                                 # shade_depth's level, and default_params'
SHADE_ALBEDO = 200                                  # shade_depth's grey
SHADE_LIGHT_CONE_DEG = 50.0                         # the light travels within this angle of the view axis
SHADE_AMBIENT_RANGE = (.10, .35)
SHADE_PALETTE = ((160, 90, 30), (128, 128, 128), (235, 235, 235), (30, 110, 240))      # BGR: industrial blue, grey, white, orange
SHADE_ALBEDO_JITTER = 18                            # levels either way, per channel
SHADE_GAIN_RANGE = (.85, 1.15)                      # per channel: white balance
SHADE_NOISE_Q_RANGE = (0, 48)                       # noise spans -+ (510 q) >> 10 levels: up to 23
SHADE_BG_DEPTH_RANGE = (3.0, 6.0)                   # metres: behind the robot's workspace as DEFAULT_CAMERA_POSE sees it
SHADE_N_BACKGROUNDS = 8                             # pictures a PhotoDataset draws its backgrounds from
