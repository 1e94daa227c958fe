"""Model zoo: LeNet (MNIST), ResNet v1.5 (50/101/152), ResNeXt (50 32x4d, 101 32x8d), BERT-base."""
from .lenet import LeNet  # noqa: F401
from .resnet import ResNet, ResNet50, ResNet152, ResNeXt50_32x4d, ResNeXt101_32x8d, SoftmaxCrossEntropyLoss  # noqa: F401
from .bert import Bert, BertPretrainingLoss, SyntheticBertLoader  # noqa: F401
