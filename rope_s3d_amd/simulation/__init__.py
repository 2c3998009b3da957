from .lookup import RobotLookupCreator
from .render import DatasetRenderer, Renderer
