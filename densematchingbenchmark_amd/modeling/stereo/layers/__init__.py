from .basic_layers import FusedConv3d, HeadConv3d, conv3d_bn, conv3d_bn_relu, deconv3d_bn  # noqa: F401
from .preact import PreActConv, SmallConvBnRelu, bn_relu_conv, bn_relu_conv3d  # noqa: F401
from .small_conv5x5 import SmallConv5x5  # noqa: F401
