from .anchor_head import AnchorHead
from .rpn_head import RPNHead
from .bbox_head import BBoxHead
from .rcnn_head import RCNNHead
from .double_head import DoubleHead
from .retina_head import RetinaHead
from .fcos_head import FCOSHead
from .guided_head import GuidedAnchor, GARPNHead

__all__ = ['AnchorHead', 'RPNHead', 'BBoxHead', 'RCNNHead', 'DoubleHead', 'RetinaHead', 'FCOSHead', 'GuidedAnchor',
           'GARPNHead']
