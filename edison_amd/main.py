#!/usr/bin/env python
"""``./main.py <module> <command> [args]`` -- the command line of the reference (audio/main.py) for the modules that sit
on the keyword-spotting hot path:

    mfcc host [wav]                      audio/main.py:80-99,199     -> edison_amd.mfcc.mfcc
    mfcc mcu calc|single|file ...        mfcc_on_mcu.py:526-548      -> edison_amd.mfcc.mfcc_on_mcu
    kws  mcu single|fileinf|file|frame   kws_on_mcu.py:650-690       -> edison_amd.kws.kws_host
    kws  live host|mcu <wav> [--net f]   audio/main.py:231-233       -> edison_amd.kws.kws_live
    kws  eval <audio.npy> <labels.npy>   nnom_utils.c:178-254        -> edison_amd.kws.kws_eval
    kws  quantize <net> <audio> <out>    kws_nnom.py:305             -> edison_amd.kws.kws_quantize
    kws  train <net> <x> <y> <out>       kws_keras.py:400-416        -> edison_amd.kws.kws_train
    kws  train --arch NAME <x> <y> <out> kws_keras.py:170-416        -> edison_amd.kws.kws_train

Where the reference talks to the STM32 board over the UART, the board's leg is computed by the GPU's bit-exact
variant C. The remaining reference modules (mic, acquire, deploy, mcu) drive the board and are out of scope; of
``train`` the engine and the model zoo are here (``kws train``: Adam, SGD or Adadelta on a float32 network, which ``--arch`` builds from
scratch as ``kws_keras.get_model`` does), not reading wav directories into data sets. One deliberate
difference: the reference's ``kws`` dispatcher runs ``live`` and then falls into the "Unrecognized command" branch of
the next ``if`` (main.py:158-165, exit status 1); here ``kws live`` returns 0.
"""
import importlib
import sys

# module -> command -> (python module under edison_amd, how many leading argv entries that module's main() skips)
COMMANDS = {
    "mfcc": {
        "host": ("edison_amd.mfcc.mfcc", 3),
        "mcu": ("edison_amd.mfcc.mfcc_on_mcu", 2),
    },
    "kws": {
        "mcu": ("edison_amd.kws.kws_host", 2),
        "live": ("edison_amd.kws.kws_live", 2),
        "eval": ("edison_amd.kws.kws_eval", 2),
        "quantize": ("edison_amd.kws.kws_quantize", 2),
        "train": ("edison_amd.kws.kws_train", 2),
    },
}

USAGE = """usage: edison <module> <command> [<args>]

  mfcc host [wav]                        MFCC variants A / B of a wav on the GPU
  mfcc mcu calc [file]                   write the firmware's mel_constants.h
  mfcc mcu single [wav] | file <wav>     host model (variant B) against the firmware's arithmetic (variant C)
  kws  mcu single [n] | fileinf <wav> | file <wav> | frame <wav>
  kws  live host|mcu <wav> [--net <file.ednf>]
                                         the firmware's continuous mode replayed on a wav (--net: the float32 X-CUBE-AI network)
  kws  eval <audio.npy> <labels.npy> [--graph <f> | --net <file.ednf>] [--geometry k=v,...] [--top-k K] [--chunk N]
                                         confusion matrix and top-k accuracy on a labelled data set, counted on the GPU
  kws  quantize <net.ednf> <audio.npy> <out.ednn> [--weights-h <out.h>] [--saturate <share>] [--geometry k=v,...] [--chunk N]
                                         quantise a float32 network to an int8 NNoM graph, calibrated on the GPU over the audio
  kws  train <net.ednf> | --arch NAME [--classes N] [--in-shape h,w,c]  <x.npy> <y.npy> <out.ednf>
             [--epochs N] [--batch N] [--lr r] [--seed s] [--val <x.npy> <y.npy>] [--opt adam|sgd|adadelta] [--rho r]
             [--resident] [--audio [--geometry k=v,...]]
             [--dropout r,.. [--dropout-before-pool b,..] | --dropout-arch NAME]
             [--batchnorm b,.. | --batchnorm-arch NAME] [--bn-momentum m] [--bn-eps e] [--bn-unbiased]
                                         train a float32 network on features and class indices: Adam on the GPU, Dropout and BatchNorm if asked;
                                         --arch: one of the reference's architectures from scratch; --resident / --audio: the data set
                                         (features, or audio whose features are computed there) lives on the device, one call an epoch
"""


class Edison(object):
    """Same shape as the reference's dispatcher class: construct with argv, read ``rc``."""

    def __init__(self, argv=None):
        self.argv = list(sys.argv if argv is None else argv)
        self.rc = self._run()

    def _run(self):
        module = self.argv[1] if len(self.argv) > 1 else None
        if module not in COMMANDS:
            print("Unrecognized module")
            print(USAGE)
            return 1
        command = self.argv[2] if len(self.argv) > 2 else None
        if command not in COMMANDS[module]:
            print("Unrecognized command")
            print(USAGE)
            return 1
        target, skip = COMMANDS[module][command]
        return importlib.import_module(target).main(self.argv[skip:])


def main(argv=None):
    return Edison(argv).rc


if __name__ == "__main__":
    sys.exit(main())
