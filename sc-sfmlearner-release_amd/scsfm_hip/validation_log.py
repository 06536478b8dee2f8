"""The validation pictures of train.py --log-output on the GPU through libscsfm_vlog.so (include/scsfm_vlog.h).

    array = tensor2array(tensor, max_value=None, colormap='rainbow')     # the reference's utils.tensor2array
    floats, rgba = map_pictures(maps, 'magma')                           # float32 [N, 4, H, W], uint8 [N, H, W, 4]
    floats, rgb = input_pictures(batch)                                  # float32 [N, 3, H, W], uint8 [N, H, W, 3]
    PictureLog(directory).add_image('val Depth Output', rgba[0], epoch)  # <directory>/val_Depth_Output/0003.png

``tensor2array`` has the reference's signature and dispatch (utils.py:42-54) and returns its float32 array bit for bit,
with matplotlib's under / over / bad rules, but takes a device tensor and leaves the result on the device: the maximum,
the division, the table lookup and the conversion to bytes all run there, and the one copy a picture costs is the copy
of its bytes in ``PictureLog.add_image``.  Host side: the three float tables ('rainbow' with 1000 entries, 'magma'
interpolated to 1000, 'bone' with 10 000), built in numpy (no matplotlib) and kept on each device after the first use,
and ``PictureLog``, the stand-in for tensorboardX's SummaryWriter that writes PNG files.  There is no CPU fallback:
without a HIP device or the library the wrappers raise.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib
from . import visualise as _visualise
from .visualise import _check_device, _ptr, _stream

# matplotlib's `magma` colour list (_cm_listed._magma_data, 256 entries of (R, G, B), CC0) in millionths, which is all
# the digits it is published with; tests/test_validation_log_reference.py compares every entry with the installed
# matplotlib
_MAGMA_MILLIONTHS = (
    "  1462    466  13866   2258   1295  18331   3279   2305  23708   4512   3490  29965   5950   4843  37130   7588 "
    "  6356  44973   9426   8022  52844  11465   9828  60750  13708  11771  68667  16156  13840  76603  18815  16026 "
    " 84584  21692  18320  92610  24792  20715 100676  28123  23201 108787  31696  25765 116965  35520  28397 125209 "
    " 39608  31090 133515  43830  33830 141886  48062  36607 150327  52320  39407 158841  56615  42160 167446  60949 "
    " 44794 176129  65330  47318 184892  69764  49726 193735  74257  52017 202660  78815  54184 211667  83446  56225 "
    "220755  88155  58133 229922  92949  59904 239164  97833  61531 248477 102815  63010 257854 107899  64335 267289 "
    "113094  65492 276784 118405  66479 286321 123833  67295 295879 129380  67935 305443 135053  68391 315000 140858 "
    " 68654 324538 146785  68738 334011 152839  68637 343404 159018  68354 352688 165308  67911 361816 171713  67305 "
    "370771 178212  66576 379497 184801  65732 387973 191460  64818 396152 198177  63862 404009 204935  62907 411514 "
    "211718  61992 418647 218512  61158 425392 225302  60445 431742 232077  59889 437695 238826  59517 443256 245543 "
    " 59352 448436 252220  59415 453248 258857  59706 457710 265447  60237 461840 271994  60994 465660 278493  61978 "
    "469190 284951  63168 472451 291366  64553 475462 297740  66117 478243 304081  67835 480812 310382  69702 483186 "
    "316654  71690 485380 322899  73782 487408 329114  75972 489287 335308  78236 491024 341482  80564 492631 347636 "
    " 82946 494121 353773  85373 495501 359898  87831 496778 366012  90314 497960 372116  92816 499053 378211  95332 "
    "500067 384299  97855 501002 390384 100379 501864 396467 102902 502658 402548 105420 503386 408629 107930 504052 "
    "414709 110431 504662 420791 112920 505215 426877 115395 505714 432967 117855 506160 439062 120298 506555 445163 "
    "122724 506901 451271 125132 507198 457386 127522 507448 463508 129893 507652 469640 132245 507809 475780 134577 "
    "507921 481929 136891 507989 488088 139186 508011 494258 141462 507988 500438 143719 507920 506629 145958 507806 "
    "512831 148179 507648 519045 150383 507443 525270 152569 507192 531507 154739 506895 537755 156894 506551 544015 "
    "159033 506159 550287 161158 505719 556571 163269 505230 562866 165368 504692 569172 167454 504105 575490 169530 "
    "503466 581819 171596 502777 588158 173652 502035 594508 175701 501241 600868 177743 500394 607238 179779 499492 "
    "613617 181811 498536 620005 183840 497524 626401 185867 496456 632805 187893 495332 639216 189921 494150 645633 "
    "191952 492910 652056 193986 491611 658483 196027 490253 664915 198075 488836 671349 200133 487358 677786 202203 "
    "485819 684224 204286 484219 690661 206384 482558 697098 208501 480835 703532 210638 479049 709962 212797 477201 "
    "716387 214982 475290 722805 217194 473316 729216 219437 471279 735616 221713 469180 742004 224025 467018 748378 "
    "226377 464794 754737 228772 462509 761077 231214 460162 767398 233705 457755 773695 236249 455289 779968 238851 "
    "452765 786212 241514 450184 792427 244242 447543 798608 247040 444848 804752 249911 442102 810855 252861 439305 "
    "816914 255895 436461 822926 259016 433573 828886 262229 430644 834791 265540 427671 840636 268953 424666 846416 "
    "272473 421631 852126 276106 418573 857763 279857 415496 863320 283729 412403 868793 287728 409303 874176 291859 "
    "406205 879464 296125 403118 884651 300530 400047 889731 305079 397002 894700 309773 393995 899552 314616 391037 "
    "904281 319610 388137 908884 324755 385308 913354 330052 382563 917689 335500 379915 921884 341098 377376 925937 "
    "346844 374959 929845 352734 372677 933606 358764 370541 937221 364929 368567 940687 371224 366762 944006 377643 "
    "365136 947180 384178 363701 950210 390820 362468 953099 397563 361438 955849 404400 360619 958464 411324 360014 "
    "960949 418323 359630 963310 425390 359469 965549 432519 359529 967671 439703 359810 969680 446936 360311 971582 "
    "454210 361030 973381 461520 361965 975082 468861 363111 976690 476226 364466 978210 483612 366025 979645 491014 "
    "367783 981000 498428 369734 982279 505851 371874 983485 513280 374198 984622 520713 376698 985693 528148 379371 "
    "986700 535582 382210 987646 543015 385210 988533 550446 388365 989363 557873 391671 990138 565296 395122 990871 "
    "572706 398714 991558 580107 402441 992196 587502 406299 992785 594891 410283 993326 602275 414390 993834 609644 "
    "418613 994309 616999 422950 994738 624350 427397 995122 631696 431951 995480 639027 436607 995810 646344 441361 "
    "996096 653659 446213 996341 660969 451160 996580 668256 456192 996775 675541 461314 996925 682828 466526 997077 "
    "690088 471811 997186 697349 477182 997254 704611 482635 997325 711848 488154 997351 719089 493755 997351 726324 "
    "499428 997341 733545 505167 997285 740772 510983 997228 747981 516859 997138 755190 522806 997019 762398 528821 "
    "996898 769591 534892 996727 776795 541039 996571 783977 547233 996369 791167 553499 996162 798348 559820 995932 "
    "805527 566202 995680 812706 572645 995424 819875 579140 995131 827052 585701 994851 834213 592307 994524 841387 "
    "598983 994222 848540 605696 993866 855711 612482 993545 862859 619299 993170 870024 626189 992831 877168 633109 "
    "992440 884330 640099 992089 891470 647116 991688 898627 654202 991332 905763 661309 990930 912915 668481 990570 "
    "920049 675675 990175 927196 682926 989815 934329 690198 989434 941470 697519 989077 948604 704863 988717 955742 "
    "712242 988367 962878 719649 988033 970012 727077 987691 977154 734536 987387 984288 742002 987053 991438 749504 ")
_MAGMA_N = 1000  # the reference's high_res_colormap(cm.get_cmap('magma')): 256 entries interpolated to 1000


@functools.lru_cache(maxsize=None)
def colour_table_f32(name):
    """float32 [N, 4]: float32 of the float64 lookup table of the reference's COLORMAPS[name]: 'rainbow' (N = 1000, the
    OpenCV-style one), 'magma' (N = 1000) or 'bone' (N = 10 000).  Read-only; any other name raises ValueError."""
    if name == "magma":
        low = np.array(_MAGMA_MILLIONTHS.split(), dtype=np.float64).reshape(256, 3) / 1e6
        x, new_x = np.linspace(0, 1, 256), np.linspace(0, 1, _MAGMA_N)
        rgba = np.stack([np.interp(new_x, x, low[:, i]) for i in range(3)] + [np.ones(_MAGMA_N)], axis=1)
    elif name in _visualise._SEGMENTS:
        n, seg = _visualise._SEGMENTS[name]
        rgba = np.stack([_visualise._channel(n, seg[c]) for c in ("red", "green", "blue")] + [np.ones(n)], axis=1)
    else:
        raise ValueError(f"unknown colour map {name!r} (known: ['bone', 'magma', 'rainbow'])")
    table = np.ascontiguousarray(rgba.astype(np.float32))
    table.setflags(write=False)
    return table


_device_tables = {}


def _table_on(name, device):
    key = (name, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(colour_table_f32(name).copy()).to(device)
    return _device_tables[key]


def _maps(maps):
    """float32 [N, H, W] or [N, 1, H, W] on the device -> contiguous [N, H, W]."""
    _check_device(maps, "maps")
    if maps.dim() == 4 and maps.shape[1] == 1:
        maps = maps[:, 0]
    if maps.dtype != torch.float32 or maps.dim() != 3 or maps.numel() < 1:
        raise ValueError("maps must be float32 [N, H, W] or [N, 1, H, W] with at least one pixel")
    return maps.contiguous()


def image_max(maps):
    """float32 [N, H, W] on the device -> float32 [N]: every image's maximum, NaN when the image holds one."""
    maps = _maps(maps)
    N, H, W = maps.shape
    with torch.cuda.device(maps.device):
        out = torch.empty(N, dtype=torch.float32, device=maps.device)
        _lib.get_vlog().call("scsfm_vlog_image_max", N, H * W, _ptr(maps), _ptr(out), _stream(maps))
    return out


def target_disparity(depth):
    """A ground-truth depth, float32 [N, H, W] on the device -> the disparity train.py shows for it (train.py:397-398 of
    the reference): 1 / depth with 1000 in the place of every 0, clamped to [0, 10].  ``depth`` is not written."""
    depth = _maps(depth)
    N, H, W = depth.shape
    with torch.cuda.device(depth.device):
        out = torch.empty_like(depth)
        _lib.get_vlog().call("scsfm_vlog_target_disparity", N, H * W, _ptr(depth), _ptr(out), _stream(depth))
    return out


def input_pictures(batch, floats=True, bytes_=True):
    """The normalised batch, float32 [N, 3, H, W] on the device -> (float32 [N, 3, H, W], uint8 [N, H, W, 3]):
    0.45 + x * 0.225 and its bytes.  An output that is not asked for is None."""
    _check_device(batch, "batch")
    if batch.dtype != torch.float32 or batch.dim() != 4 or batch.shape[1] != 3 or batch.numel() < 1:
        raise ValueError("batch must be float32 [N, 3, H, W] with at least one pixel")
    if not (floats or bytes_):
        raise ValueError("at least one output must be asked for")
    batch = batch.contiguous()
    N, _, H, W = batch.shape
    with torch.cuda.device(batch.device):
        out_f = torch.empty_like(batch) if floats else None
        out_b = torch.empty((N, H, W, 3), dtype=torch.uint8, device=batch.device) if bytes_ else None
        _lib.get_vlog().call("scsfm_vlog_input_picture", N, H, W, _ptr(batch), _ptr(out_f), _ptr(out_b), _stream(batch))
    return out_f, out_b


def map_pictures(maps, colormap='rainbow', max_value=None, floats=True, bytes_=True):
    """float32 [N, H, W] or [N, 1, H, W] on the device -> (float32 [N, 4, H, W], uint8 [N, H, W, 4]): per image the
    reference's ``tensor2array(map, max_value, colormap)`` and its bytes.  ``max_value=None`` divides every image by its
    own maximum (found on the device, no host round trip).  An output that is not asked for is None."""
    table = colour_table_f32(colormap)
    if not (floats or bytes_):
        raise ValueError("at least one output must be asked for")
    maps = _maps(maps)
    N, H, W = maps.shape
    with torch.cuda.device(maps.device):
        divisors = image_max(maps) if max_value is None else None
        dev_table = _table_on(colormap, maps.device)
        out_f = torch.empty((N, 4, H, W), dtype=torch.float32, device=maps.device) if floats else None
        out_b = torch.empty((N, H, W, 4), dtype=torch.uint8, device=maps.device) if bytes_ else None
        _lib.get_vlog().call("scsfm_vlog_map_picture", N, H, W, _ptr(maps), _ptr(dev_table), len(table), _ptr(divisors),
                             0.0 if max_value is None else float(max_value), _ptr(out_f), _ptr(out_b), _stream(maps))
    return out_f, out_b


def tensor2array(tensor, max_value=None, colormap='rainbow'):
    """The reference's utils.tensor2array on a device tensor: [H, W] or [1, H, W] -> float32 [4, H, W] (the map over
    ``max_value``, or over its own maximum, in ``colormap``); [3, H, W] -> float32 [3, H, W] (the de-normalised input).
    The result stays on the device."""
    tensor = tensor.detach()
    if tensor.dim() == 2 or tensor.size(0) == 1:
        one = tensor if tensor.dim() == 2 else tensor[0]
        if one.dim() != 2:
            raise ValueError("a map must be [H, W] or [1, H, W]")
        return map_pictures(one[None], colormap, max_value, bytes_=False)[0][0]
    if tensor.dim() == 3:
        assert tensor.size(0) == 3
        return input_pictures(tensor[None], bytes_=False)[0][0]
    raise ValueError("tensor must be [H, W], [1, H, W] or [3, H, W]")


def to_bytes(array):
    """The byte rule of include/scsfm_vlog.h in numpy: uint8(min(max(float32(255) * float32(v), 0), 255)), NaN -> 0."""
    t = np.float32(255) * np.asarray(array, dtype=np.float32)
    t = np.where(t > 0, t, np.float32(0))
    return np.where(t < 255, t, np.float32(255)).astype(np.uint8)


class PictureLog(object):
    """Stand-in for tensorboardX.SummaryWriter(directory) as train.py --log-output uses it (train.py:88-90 of the
    reference; the package is absent here): ``add_image(tag, picture, step)`` writes
    ``<directory>/<tag with spaces as '_'>/<step:04d>.png``, RGBA for four channels and RGB for three."""

    def __init__(self, directory):
        self.directory = str(directory)

    def path(self, tag, step):
        return os.path.join(self.directory, tag.replace(" ", "_"), "{:04d}.png".format(int(step)))

    def add_image(self, tag, picture, step=0):
        """``picture``: uint8 [H, W, C] (on the device: this is the one copy the picture costs) or a float [C, H, W]
        array or tensor in [0, 1], which goes through the same byte rule; C is 3 or 4."""
        from PIL import Image
        if isinstance(picture, torch.Tensor):
            picture = picture.detach().cpu().numpy()
        picture = np.asarray(picture)
        if picture.dtype != np.uint8:
            picture = np.ascontiguousarray(to_bytes(picture).transpose(1, 2, 0))
        if picture.ndim != 3 or picture.shape[2] not in (3, 4):
            raise ValueError("a picture is uint8 [H, W, C] or float [C, H, W] with 3 or 4 channels")
        path = self.path(tag, step)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(np.ascontiguousarray(picture)).save(path)  # (uint8 [H, W, 3 / 4]: RGB / RGBA)
        return path
