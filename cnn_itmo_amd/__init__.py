"""cnn_itmo_amd -- MI355X-native (gfx950) CNN-ITMO SDR->HDR U-Net hot path.

Keras-compatible front end (layers, Model, U_net, ConvBN, ConvBNTranspose,
load_model) over hand-written HIP kernels in lib/libcnnitmo.so (C ABI:
include/cnn_itmo.h).  No CPU fallback: the engine raises without a ROCm GPU.
"""
from .layers import (Activation, BatchNormalization, Concatenate, Conv2D, Conv2DTranspose, Dropout,
                     Input, InputLayer, MaxPooling2D, clear_session, concatenate)
from .model import Model, load_model
from .optimizers import SGD, Adam, RMSprop
from .losses import DSSIM, MSSSIM, HighlightWeighted
from .unet import ConvBN, ConvBNTranspose, TinyNet, U_net
from .callbacks import (CSVLogger, EarlyStopping, LambdaCallback, LearningRateScheduler, ModelCheckpoint,
                        ReduceLROnPlateau, TerminateOnNaN)
from . import degrade, exr, hdrio, hdrmetrics, metrics, resize
from .hdrgen import HDRPairGenerator, HDRPairIterator

__all__ = ["HDRPairGenerator", "HDRPairIterator","Activation", "BatchNormalization", "Concatenate", "Conv2D", "Conv2DTranspose", "Dropout",
           "Input", "InputLayer", "MaxPooling2D", "clear_session", "concatenate", "Model", "RMSprop",
           "Adam", "SGD", "DSSIM", "MSSSIM", "HighlightWeighted", "load_model", "ConvBN", "ConvBNTranspose", "TinyNet", "U_net", "CSVLogger",
           "LambdaCallback", "ModelCheckpoint", "LearningRateScheduler", "ReduceLROnPlateau", "EarlyStopping",
           "TerminateOnNaN", "metrics", "hdrio", "hdrmetrics", "degrade", "resize", "exr"]
