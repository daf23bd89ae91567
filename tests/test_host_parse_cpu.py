"""C++ host: what every argument of the IR options and index lines parses to is on record.  Convolution's static parsers (conv.h:
parseTail, parsePhase, parseFilter, parseMatch, parseParts for --ir-* options, parseSynth, parseRoom, parsePlate, parseSpring,
parseSweep for index lines, and the one-value parseDensity, parseIacc, parseSti, parseResponse) turn text into structs; the other
host tests pin that a malformed argument is refused with a message that names the key, by substring, and none pins what an
accepted one becomes.  tests/stub/parse_dump.cpp prints, for one grammar and one argument, "ok" or "refused", the reason and every
member of the struct; tests/golden/host_parse.json holds that line for every case below, as the parsers of the commit its "commit"
field names printed it.  The test builds the driver against the tree under test (the Makefile's mcconv_parse_dump, which links the
parsers without conv.o or an engine), runs every case and compares the whole line for equality.

The fixture stores text, not digests, and stores it short, since a room's line alone is over a kilobyte.  Per grammar it holds
the form the refusals quote ("form"), the members a refused argument leaves behind ("refused": the default-constructed struct) and
the members of the grammar's plain argument ("accepted": BASE's parse).  An accepted case is stored as `ok` and the members that
differ from "accepted", which is what its items moved: `ok floorDb=90.5 overLog2=6`.  A refused case is stored as `refused` and
the reason, with the form as `<form>`.  In a case's name `~` stands for BASE.  expand() puts all of it back and the comparison is on
the driver's whole line.  One line of the file holds one group of cases: a key's values, the list structure, the fields, the rest.

The cases are literal data and a few loops; nothing is random.  Per key: a typical value, each bound, the nearest value outside
it, the forms of NUMS, the key given twice.  Per grammar: the structure cases, the cross-key rules, the bare words and every
argument the other host tests hand to that parser.  Two conditions hold over the fixture itself, so that it cannot hide a
mis-wired key: for every key an accepted case differs from the same argument without that item, and for every key a case is
refused.

The fixture is recorded by this module run as a program, from a build of the commit to record:
    python tests/test_host_parse_cpu.py <output.json> <the commit that build is of> <its parse_dump binary>
The test itself never records and never skips."""
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "cuda_audio_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_parse.json")

ROOM = "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5"
SWEEP = "sweep:rec.wav:0.1:100:20000"
# what a list of items is appended to (parts has nothing before its list)
BASE = {"tail": "extend", "phase": "minimum", "filter": "f.wav", "match": "t.wav", "parts": "", "synth": "synth:1.0:0.5", "room": ROOM,
        "plate": "plate:0.2", "spring": "spring:0.2", "sweep": SWEEP}
ONE_VALUE = ("density-window", "density-hop", "density-t60", "iacc-lag", "iacc-bands", "sti-snr", "response-smooth")
WHOLE = ("iacc-lag", "iacc-bands", "sti-snr")  # their structs hold a vector whose elements come and go: every member of an accepted case is stored
NUMS = ("x", "", "nan", "inf", "1e3", "0x10", " 1", "+1", "-0")
SEEDS = ("-1", " -1", "0x10", "010", "18446744073709551616", "18446744073709551615", "1.5")


def K(key, typical, second, edges=(), more=(), ctx=""):
    """A key: a typical value (not the default), another for `key=typical,key=second`, (bound, nearest outside) pairs, further
    values, and the items that have to stand before it for it to be accepted."""
    return dict(key=key, typical=typical, second=second, edges=edges, more=more, ctx=ctx)


GE0 = (("0", "-1e-9"),)
SYNTH_KEYS = [
    K("seed", "7", "9", more=SEEDS),
    K("start", "0.01", "0.02", GE0),
    K("buildup", "0.0125", "0.02", GE0),
    K("late", "0.05", "0.5", GE0),
    K("direct", "1", "-0.5", more=("-1e30",)),
    K("early", "6", "3", (("0", "-1"), ("64", "65")), more=("2.5", "64.0", "6e0")),
    K("efirst", "0.001", "0.002", GE0),
    K("elast", "0.009", "0.01", GE0),
    K("egain", "0.5", "-2", more=("-1e30",)),
    K("width", "0.7", "0.2", (("0", "-1e-9"), ("1", "1.000000001"))),
]
KEYS = {
    "tail": [
        K("fade", "0.005", "0.1", (("0", "-1e-9"), ("4000", "4000.0001"))),
        K("length", "1.5", "2", (("0", "-1e-9"), ("4000", "4000.0001"))),
        K("seed", "3", "9", more=SEEDS),
        K("width", "0.5", "0.25", (("0", "-1e-9"), ("1", "1.000000001")), more=("iacc", "IACC", "iac")),
        K("knee", "mix", "floor", more=("floor", "mixing", "0.5")),
    ],
    "phase": [
        K("floor", "90.5", "100", (("40", "39.999999"), ("300", "300.000001"))),
        K("over", "64", "2", (("2", "1"), ("64", "128")), more=("3", "4", "8", "16", "32", "8.5", "0", "-2", "2.0", "6.4e1")),
    ],
    "filter": [
        K("op", "deconvolve", "convolve", more=("convolve", "divide", "Deconvolve")),
        K("channels", "mid", "left", more=("stereo", "left", "right", "0")),
        K("reg", "90.5", "40", (("20", "19.999999"), ("200", "200.000001"))),
        K("keep", "0.25", "2", (("1e-300", "0"), ("3600", "3600.000001")), more=("-1",)),
    ],
    "match": [
        K("amount", "0.5", "0.25", (("0", "-1e-9"), ("1", "1.000000001"))),
        K("boost", "6", "3", (("0", "-1e-9"), ("60", "60.000001"))),
        K("cut", "9", "4", (("0", "-1e-9"), ("60", "60.000001"))),
        K("smooth", "0.5", "1", (("0.041666666666666664", "0.04166666666666666"), ("2", "2.000000001"))),
        K("lo", "30", "40", (("1", "0.999999999"), ("192000", "192000.0001"))),
        K("hi", "3000", "3500", (("1", "0.999999999"), ("192000", "192000.0001")), more=("20", "20.000001", "0")),
        K("link", "0", "1", more=("1", "2", "true", "00")),
        K("phase", "linear", "minimum", more=("minimum", "maximum", "Linear")),
        K("delay", "0.01", "0.02", (("0", "-1e-9"), ("10", "10.000000001"))),
        K("tilt", "-3", "3", (("-12", "-12.000001"), ("12", "12.000001"))),
    ],
    "parts": [
        K("direct", "-3", "-6", (("-120", "-120.0001"), ("24", "24.0001")), more=("off", "Off", "loud", "0:0")),
        K("early", "-4", "-6", (("-120", "-120.0001"), ("24", "24.0001")), more=("off", "0:0")),
        K("late", "2", "-6", (("-120", "-120.0001"), ("24", "24.0001")), more=("off", "0:0")),
        K("split", "0.05", "0.06", (("0", "-1e-9"), ("100", "100.000001")), more=("mix", "Mix", "soon", "0.001", "0.0025", "0.1:0.1"), ctx="first=0"),
        K("first", "0.002", "0.003", (("0", "-1e-9"), ("100", "100.000001")), more=("0.08", "0.080001"), ctx="split=100"),
        K("onset", "0.001", "0.002", (("0", "-1e-9"), ("100", "100.000001"))),
        K("xfade", "0.001:0.01", "0.002:0.02", (("0:0", "0:-1e-9"), ("100:100", "100:100.000001")), more=("0.01", "0.01:0.01:0.01", "0.01:", ":0.01", "0.01:x", "nan:0")),
        K("delay", "0:0.001:-0.002", "0.1:0.1:0.1", (("-10:-10:-10", "-10:-10:-10.000001"), ("10:10:10", "10.000001:10:10")),
          more=("0.1", "0:0", "0:0:0:0", "0:0:x", "0::0", "0:0:inf")),
        K("width", "1:0.3:1.7", "0.5", (("0", "-1e-9"), ("2", "2.000000001")), more=("0:0:0", "2:2:2", "1:1", "1:1:-1", "1:1:1:1", "1:x:1")),
        K("balance", "0.25", "-0.5:0:0.5", (("-1", "-1.000000001"), ("1", "1.000000001")), more=("-1:0:1", "0:0:0:0", "0:0", "0:0:1.5")),
        K("swap", "early", "late", more=("direct", "direct:early:late", "early:early", "middle", "direct:", ":direct", "Direct")),
        K("invert", "direct:late", "early", more=("late", "direct:early:late", "middle", "direct:", "late:tail")),
    ],
    "synth": SYNTH_KEYS,
    "room": [
        K("beta", "0.8", "0.7", more=("0.9/0.8/0.7/0.95/0.6/0.85", "0.9/0.8", "0.9/0.8/0.7/0.6/0.5/x", "0.9/0.8/0.7/0.6/0.5/0.4/0.3", "-1", "2", "/", "0.9/")),
        K("order", "5", "7", (("0", "-1"), ("32", "33")), more=("2.5", "5.0")),
        K("spacing", "0.3", "0.1", GE0),
        K("axis", "y", "z", more=("x", "z", "w", "X", "xy", "1")),
        K("speed", "340", "330", GE0),
        K("gain", "0.2", "2", GE0),
        K("last", "0.1", "0.15", GE0),
        K("t60", "0.3", "0.4", GE0),
        K("mic", "cardioid", "fig8/0.75", (("0", "-1e-9"), ("1", "1.000000001")),
          more=("omni", "subcardioid", "supercardioid", "hypercardioid", "fig8", "0.5/0.25", "omni/fig8", "shotgun", "cardioid/", "/cardioid", "0.5/0.5/0.5", "0.5/1.5")),
        K("aim", "45/-45", "200", (("-360", "-360.000001"), ("360", "360.000001")), more=("north", "45/-361", "45/", "1/2/3", "360/-360")),
        K("tilt", "10", "5/-5", (("-90", "-90.000001"), ("90", "90.000001")), more=("91", "10/nan", "90/-90")),
        K("src", "hypercardioid", "0.25", (("0", "-1e-9"), ("1", "1.000000001")), more=("omni", "cardioid", "fig8", "cardioid/cardioid", "Cardioid")),
        K("srcaim", "-30", "30", (("-360", "-360.000001"), ("360", "360.000001")), more=("400", "1/2")),
        K("srctilt", "5", "-5", (("-90", "-90.000001"), ("90", "90.000001")), more=("-90.5", "up")),
        K("xover", "500/2000", "1000", (("10", "9.999999"), ("172800", "172800.1")),
          more=("500", "250/1000/4000", "low", "5", "500/", "2000/500", "500/500", "100/200/300/400", "10/172800", "/500")),
        K("betas", "0.9/0.8/0.6", "0.7/0.6/0.5", (("-1/-1/-1", "-1/-1/-1.000001"), ("1/1/1", "1.000001/1/1")),
          more=("hard", "0.9", "0.9/0.8", "0.9/0.8/0.7/0.6", "0.9/0.8/0.7/0.6/0.5", "0.9/0.8/"), ctx="xover=500/2000"),
        K("air", "0/0.005/0.03", "0.01", (("0", "-1e-9"), ("1", "1.000001")),
          more=("0.02", "1/1/1", "0/0/1.5", "thin", "0/0.1", "0/0.1/0.2/0.3", "0/0.1/"), ctx="xover=500/2000"),
        K("head", "35", "-120", (("-360", "-360.000001"), ("360", "360.000001")), more=("north", "10/20")),
        K("headradius", "0.09", "0.08", (("0.05", "0.049999"), ("0.15", "0.150001")), more=("0.04", "0.2")),
        K("ears", "100", "80", (("60", "59.999999"), ("120", "120.000001"))),
        K("shadow", "0.8", "0.5", (("0", "-1e-9"), ("1", "1.000000001")), more=("deep",)),
    ] + SYNTH_KEYS,
    "plate": [
        K("size", "1.5,0.8", "2,1", (("0,0", "0,-1e-9"),), more=("2", "2,1,3", "2,x", "2/1", ",1", "2,", "nan,1")),
        K("thick", "1", "2", GE0, more=("thin",)),
        K("material", "70/2700/0.33", "steel", (("0/0/0", "0/0/-1e-9"),), more=("steel", "Steel", "brass", "200/7850", "200/7850/0.3/1", "200,7850,0.3", "200//0.3")),
        K("drive", "0.5,0.3", "0.5,0.25", (("0,0", "-1e-9,0"),), more=("0.5", "0.5/0.4", "0.5,0.3,0.1")),
        K("pick", "0.2,0.2/1.2,0.6", "0.3,0.3/1,0.5", (("0,0/0,0", "0,0/0,-1e-9"),), more=("0.3,0.6", "0.3,0.6/1.5", "0.3/0.6/1.5/0.3", "0.3,0.6/1.5,0.3/1,1", "/")),
        K("low", "30", "40", GE0),
        K("high", "1200", "400", GE0),
        K("t60", "0.5/0.1", "0/0", (("0/0", "0/-1e-9"),), more=("4", "4,1", "4/-1", "4/1/1")),
        K("damp", "1200", "5000", GE0),
        K("gain", "0.02", "2", GE0, more=("1,5",)),
        K("last", "0.1", "0.15", GE0),
    ],
    "spring": [
        K("sections", "40", "60", (("0", "-1"), ("1000000", "1000001")), more=("many", "1.5", "40.0")),
        K("fc", "3000", "2500", GE0),
        K("a", "0.5", "0.4", GE0, more=("-0.5",)),
        K("delay", "21,27.5,33", "30", (("1e-300", "0"),), more=("30", "66,82", "66,x", "66,82,91,100", "66,0", "66/82", "66,,82", "-1", "66,82,-1")),
        K("t60", "0.4", "0", GE0),
        K("damping", "0.1", "0.3", GE0),
        K("lowpass", "4", "0", (("0", "-1"), ("1000000", "1000001")), more=("2.5",)),
        K("high", "0.2", "0", GE0),
        K("highsections", "60", "80", (("0", "-1"), ("1000000", "1000001")), more=("2.5",)),
        K("higha", "-0.5", "-0.4", (("0", "1e-9"),), more=("0.5", "-1e30")),
        K("highdelay", "0.4", "0.3", GE0),
        K("hight60", "0.2", "0.3", GE0),
        K("stereo", "0.05", "0.1", GE0, more=("wide",)),
        K("gain", "0.02", "2", GE0, more=("1,5",)),
        K("points", "14", "20", (("0", "-1"), ("1000000", "1000001")), more=("-3", "14.5")),
        K("last", "0.1", "0.15", GE0),
    ],
    "sweep": [
        K("amp", "0.25", "0.3", (("1e-300", "0"),), more=("-0.5",)),
        K("fadein", "0.001", "0.002", (("0", "-1e-9"), ("0.1", "0.100001"))),
        K("fadeout", "0.0005", "0.002", (("0", "-1e-9"), ("0.1", "0.100001"))),
        K("offset", "-0.002", "0.01", more=("-1e30", "1e30")),
        K("length", "0.02", "0.03", GE0),
    ],
}
# the one-value options: a typical value, the bounds with the nearest value outside, and further arguments
ONE = {
    "density-window": ("0.02", (("1e-300", "0"), ("4000", "4000.0001")), ("0.0101", "0.01", "abc", "-0.01", "0.02s", "0.02,0.01", "5000", "auto", "0.0005")),
    "density-hop": ("0.0025", (("1e-300", "0"), ("4000", "4000.0001")), ("0.001", "abc", "-0.01", "0.02s", "0.02,0.01", "5000", "auto")),
    "density-t60": ("0.3", (("1e-300", "0"), ("4000", "4000.0001")), ("auto", "Auto", "abc", "-0.01", "0.02s", "0.02,0.01", "5000")),
    "iacc-lag": ("0.002", (("0", "-1e-9"), ("1", "1.000000001")), ("0.001", "0.00206", "0.2", "abc", "-0.001", "0.001s", "0.001,0.002", "1.5")),
    "iacc-bands": ("500,1000", (("1e-30", "0"),),
                   ("1000", "500,2000", "abc", "1000,", ",1000", "1000;2000", "-250", "1000,x", "1,2,3,4,5,6,7,8,9,10", "1,2,3,4,5,6,7,8,9,10,11", "1000, 2000", "1e39")),
    "sti-snr": ("10", (("-60", "-60.0001"), ("120", "120.0001")),
                ("6", "15", "-60,0,10,20,30,40,120", "abc", "10,", ",10", "10;20", "10dB", "-61", "121", "10,20", "1,2,3,4,5,6", "1,2,3,4,5,6,7,8", "1,2,3,x,5,6,7",
                 "1,2,3,4,5,6,121")),
    "response-smooth": ("0.5", (("0", "-1e-9"), ("10", "10.000000001")), ("0.333", "0.3333", "abc", "1,", "1 octave", "-0.5", "10.5", "1/3", "0x")),
}
# the positional fields of the index lines (and the option's first field), with what each is replaced by
FIELDS = {
    "tail": (["extend"], {0: ("cut", "extend", "shorten", "fade", "Cut", "")}),
    "phase": (["minimum"], {0: ("minimum", "linear", "min", "Minimum", "")}),
    "filter": (["f.wav"], {0: ("f.wav", "dir/f.wav", "")}),
    "match": (["t.wav"], {0: ("t.wav", "flat", "Flat", "")}),
    "synth": (["synth", "1.0", "0.5"], {0: ("Synth", "room"), 1: ("0.15", "abc", "0", "-1", "1e-300") + NUMS, 2: ("0.1", "0", "-0.5", "0.5x", "-1e-9") + NUMS}),
    "room": (ROOM.split(":"), {0: ("Room", "synth"), 1: ("0.1", "abc", "0", "-1") + NUMS, 2: ("6,5,2.5", "5,4", "5,4,3,2", "5,x,3", "5,,3", "-5,4,3", "5/4/3", "nan,4,3", ""),
                               3: ("2,2,1", "1,x,1.2", "1,1.5", "inf,1,1", ""), 4: ("4,3,1.5", "3.5,2,1.5,7", "3.5,2", " 3.5,2,1.5", "")}),
    "plate": (["plate", "0.2"], {0: ("Plate",), 1: ("0.15", "abc", "0", "-1") + NUMS}),
    "spring": (["spring", "0.2"], {0: ("Spring",), 1: ("0.15", "abc", "0", "-1") + NUMS}),
    "sweep": (SWEEP.split(":"), {0: ("Sweep",), 1: ("dir/rec.wav", ""), 2: ("0.085", "abc", "0", "-1") + NUMS, 3: ("20", "1", "0.5", "0.999999", "20000", "abc") + NUMS,
                                  4: ("100", "100.0001", "3500", "20000x", "99") + NUMS}),
}
# what the other host tests hand to the parsers, and the cross-key rules, orders and bare words
LITERAL = {
    "tail": ["", "fade", "extend:", "shorten", "cut:fade", "cut:fade=", "cut:=3", "extend:fade=abc", "extend:fade=-0.1", "extend:length=nan", "extend:seed=-1",
             "extend:seed=1.5", "extend:width=1.5", "extend:colour=3", "extend:fade=0.1,", "extend:fade=0.1:seed=2", "extend:knee", "extend:knee=", "extend:knee=mixing",
             "extend:knee=0.5", "cut:knee=mix", "extend:knee=mix,", "extend:width=", "extend:width=IACC", "extend:width=iac", "cut:width=iacc", "extend:width=iacc,",
             "extend:knee=floor", "extend:fade=0.005,knee=mix", "extend:width=0.5", "extend:fade=0.005,width=iacc", "extend:fade=0.005,length=1,seed=3,width=0.5", "cut",
             "extend", "extend:knee=mix", "extend:fade=0.01,length=0.5,seed=5,knee=mix", "extend:fade=0.01,length=0.5,seed=5,width=iacc", "extend:fade=0.01,seed=5",
             "extend:fade=0.01,length=0.5,seed=5",
             # the cross-key rules, with the keys around them in either order
             "cut:knee=floor", "cut:knee=mix,fade=0.1", "cut:fade=0.1,knee=mix", "cut:width=iacc,knee=mix", "cut:knee=mix,width=iacc", "cut:width=0.5", "cut:width=iacc,width=0.5",
             "extend:width=iacc,width=0.5", "extend:width=0.5,width=iacc", "cut:knee=mix,knee=floor", "cut:knee=mix,colour=3", "cut:fade=0.1,length=2,seed=4",
             "extend:knee=mix,width=iacc,seed=3,length=1,fade=0.005", "cut:seed=3,fade=0.005"],
    "phase": ["", "linear", "minimum:", "min", "minimum:floor", "minimum:floor=", "minimum:=3", "minimum:floor=abc", "minimum:floor=39", "minimum:floor=301",
              "minimum:floor=nan", "minimum:over=1", "minimum:over=3", "minimum:over=128", "minimum:over=8.5", "minimum:colour=3", "minimum:over=8,",
              "minimum:floor=100:over=8", "minimum", "minimum:floor=90.5,over=64", "minimum:over=2", "minimum:floor=100,over=4", "minimum:over=4,floor=100",
              "minimum:colour=x", "minimum:colour=nan"],
    "filter": ["f.wav" + t for t in ("", ":", ":op", ":op=", ":=deconvolve", ":op=divide", ":channels=right", ":reg=abc", ":reg=19", ":reg=201", ":reg=nan", ":keep=0",
                                     ":keep=-1", ":keep=inf", ":colour=3", ":op=convolve,", ":op=convolve:reg=60", ":op=deconvolve,channels=mid,reg=90.5,keep=0.25",
                                     ":channels=left", ":op=deconvolve,channels=mid,reg=40,keep=0.25", ":keep=0.25,reg=40,channels=mid,op=deconvolve", ":colour=abc")]
              + ["", ":", ":op=deconvolve", "nowhere.wav:op=deconvolve"],
    "match": ["t.wav" + t for t in ("", ":", ":amount", ":amount=", ":=1", ":amount=2", ":amount=-0.1", ":boost=61", ":cut=abc", ":smooth=0.01", ":smooth=3", ":lo=0.5",
                                    ":lo=500,hi=400", ":link=2", ":phase=maximum", ":delay=-1", ":delay=inf", ":tilt=13", ":tilt=nan", ":colour=3", ":amount=1,",
                                    ":amount=1:boost=3", ":amount=0.5,boost=6,cut=9,smooth=0.5,lo=30,hi=3000,link=0,phase=linear,delay=0.01",
                                    ":amount=0.5,boost=3,cut=4,smooth=0.5,lo=40,hi=3500,link=0", ":delay=0.01,phase=linear,link=0,hi=3000,lo=30,smooth=0.5,cut=9,boost=6,amount=0.5",
                                    # hi is not above lo, either order, and hi=0 (which switches the rule off)
                                    ":hi=400,lo=500", ":lo=500,hi=500", ":hi=19", ":hi=20", ":hi=0", ":lo=500,hi=0", ":hi=400,lo=500,colour=3", ":colour=abc")]
             + ["", ":", ":amount=1", "flat", "flat:tilt=-3,link=1,phase=minimum", "flat:tilt=-3,phase=linear,delay=0.01", "nowhere.wav:amount=0.5", "flat:", "flat:colour=3"],
    "parts": ["", ",", "direct", "direct=", "=3", "direct=25", "early=-121", "late=loud", "late=nan", "direct=off,early=off,late=off", "split=-1", "split=soon", "split=0.001",
              "first=abc", "onset=-0.1", "xfade=0.01", "xfade=0.01:0.01:0.01", "xfade=0.01:-1", "delay=0.1", "delay=0:0:11", "delay=0:0:x", "width=2.5", "width=1:1",
              "width=1:1:-1", "balance=1.5", "balance=0:0:0:0", "swap=middle", "invert=direct:", "colour=3", "direct=0,", "direct=0,,late=0", "swap=early,invert=late:tail",
              "direct=off",
              "direct=-3,early=-4,late=2,split=0.05,first=0.002,onset=0.001,xfade=0.001:0.01,delay=0:0.001:-0.002,width=1:0.3:1.7,balance=0.25,swap,invert=direct:late",
              "early=off,split=mix",
              "direct=-3,early=-4,late=2,split=0.05,first=0.002,onset=0.001,xfade=0.001:0.01,delay=0:0.001:-0.002,width=1:0.3:1.7,balance=0.25,swap=early,invert=direct:late",
              "direct=0,early=-3,late=-6", "direct=0,early=-3,late=-6,split=mix",
              # the bare words, split before first in either order, every part off and then one on again
              "swap", "invert", "swap,invert", "invert,swap=early", "swap=", "invert=", "swap,", "Swap", "swap,direct=0", "split=0.001,first=0.0005", "first=0.0005,split=0.001",
              "first=0.1", "first=0.1,split=mix", "split=mix,first=0.1", "split=mix,split=0.001", "split=0.001,split=mix", "direct=off,early=off,late=off,late=0",
              "direct=off,direct=0", "late=off,early=off,direct=off,colour=3", "split=0.001,colour=3",
              "invert=direct:late,swap=early,balance=0.25,width=1:0.3:1.7,delay=0:0.001:-0.002,xfade=0.001:0.01,onset=0.001,first=0.002,split=0.05,late=2,early=-4,direct=-3"],
    "synth": ["synth:", "synth:1.0", "synth:abc:0.5", "synth:0:0.5", "synth:-1:0.5", "synth:1.0:-0.5", "synth:1.0:0.5x", "synth:1.0:0.5:", "synth:1.0:0.5:seed",
              "synth:1.0:0.5:seed=-3", "synth:1.0:0.5:seed=7,", "synth:1.0:0.5:colour=3", "synth:1.0:0.5:early=65", "synth:1.0:0.5:early=2.5", "synth:1.0:0.5:width=1.5",
              "synth:1.0:0.5:late=-0.1", "synth:1.0:0.5:direct=nan", "synth:1.0:0.5:early=3,efirst=0.02,elast=0.01", "synth:1.0:0.5:seed=1:width=0.5",
              "synth:0.15:0.1:seed=0x500000007,start=0.01,buildup=0.0125,late=0.05,direct=1,early=6,efirst=0.001,elast=0.009,egain=0.5,width=0.7",
              "synth:0.25:0.2:seed=3,early=4,efirst=0.005,elast=0.05", "synth:0.5:0.3", "synth:0.5:0",
              # elast before efirst: only with reflections, in either order
              "synth:1.0:0.5:efirst=0.02,elast=0.01", "synth:1.0:0.5:early=0,efirst=0.02,elast=0.01", "synth:1.0:0.5:elast=0.01,efirst=0.02,early=3",
              "synth:1.0:0.5:early=3,efirst=0.02", "synth:1.0:0.5:early=3,efirst=0.02,elast=0.02", "synth:1.0:0.5:early=3,efirst=0.02,elast=0.01,colour=3",
              "synth:0.15:0.1:width=0.7,egain=0.5,elast=0.009,efirst=0.001,early=6,direct=1,late=0.05,buildup=0.0125,start=0.01,seed=0x500000007"],
    "room": ["room:", "room:0.2:5,4,3:1,1.5,1.2", "room:abc:5,4,3:1,1.5,1.2:3.5,2,1.5", "room:0:5,4,3:1,1.5,1.2:3.5,2,1.5", "room:0.2:5,4:1,1.5,1.2:3.5,2,1.5",
             "room:0.2:5,4,3:1,x,1.2:3.5,2,1.5", "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5,7",
             "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,spacing=0.3,axis=y", "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2", "room:0.25:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8",
             "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:gain=0.2,spacing=0.3,axis=y,xover=500/2000,betas=0.9/0.8/0.6,air=0/0.005/0.03",
             "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,beta=0.9/0.8/0.7/0.95/0.6/0.85,air=0.02,xover=1000,mic=cardioid,aim=45/-45",
             "room:0.1:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,head=35,ears=100,headradius=0.09,shadow=0.8", "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,head=-120,shadow=0.5",
             "room:0.2:5,4,3:1,1.5,1.2:3.5,2,1.5:beta=0.8,gain=0.2,axis=y,mic=cardioid,aim=45/-45,spacing=0",
             "room:0.1:6,5,2.5:2,2,1:4,3,1.5:gain=0.2,mic=fig8/0.75,tilt=10,aim=200,src=hypercardioid,srcaim=-30,srctilt=5"]
            + [ROOM + ":" + t for t in (
                "", "beta", "beta=0.9/0.8", "beta=0.9/0.8/0.7/0.6/0.5/x", "order=33", "order=2.5", "spacing=-0.1", "axis=w", "speed=fast", "gain=nan", "last=-1", "t60=-1",
                "colour=3", "late=-0.1", "early=65", "beta=0.8,", "beta=0.8:gain=2", "xover=low", "xover=5", "xover=500/", "xover=2000/500", "xover=500/500",
                "xover=100/200/300/400", "xover=nan", "betas=1.5", "betas=hard", "betas=0.9/0.8", "betas=0.9/0.8/0.7,xover=500", "xover=500/2000,betas=0.9",
                "betas=0.9/0.8/0.7/0.6/0.5", "air=-0.1", "air=1.5", "air=thin", "air=0/0.1", "xover=500/2000,air=0/0.1", "xover", "xovers=500",
                "xover=500/2000,betas=0.9/0.8/0.6,air=0/0.005/0.03", "air=0.01", "betas=0.8", "xover=1000,mic=cardioid", "head=north", "head=361", "head=10/20",
                "headradius=0.04", "headradius=0.2", "headradius=", "ears=59", "ears=121", "ears=nan", "shadow=-0.1", "shadow=1.5", "shadow=deep", "head", "heads=35",
                "head=35,ears=100", "headradius=0.08", "shadow=0", "mic=shotgun", "mic=1.5", "mic=cardioid/", "mic=0.5/0.5/0.5", "aim=north", "aim=45/-361", "tilt=91",
                "tilt=10/nan", "src=-0.1", "src=cardioid/cardioid", "srcaim=400", "srcaim=1/2", "srctilt=-90.5", "srctilt=up", "mic", "mics=cardioid",
                "mic=cardioid,aim=45/-45,spacing=0", "src=cardioid", "srctilt=0",
                # the counts of betas and air against xover's, in either order, alone and with an unknown key (which is named later)
                "betas=0.9/0.8,xover=500", "xover=500,betas=0.9/0.8", "air=0/0.1,xover=500", "xover=500,air=0/0.1", "betas=0.9/0.8,air=0/0.1", "betas=0.9/0.8,colour=3",
                "air=0/0.1,colour=3", "betas=0.9/0.8,air=0/0.1/0.2,colour=3", "xover=500,betas=0.9/0.8/0.7,air=0/0.1", "xover=500,betas=0.9/0.8,air=0/0.1/0.2", "betas=0.9,colour=3",
                "xover=500,betas=0.9/0.8,xover=500/2000", "betas=0.9/0.8,early=65", "colour=3,betas=0.9/0.8", "colour=3,gain=nan",
                # the late field's keys: late= and direct= given after the room's own win, t60 goes to the late field, its refusals carry the room's form
                "t60=0.3,late=0.5,direct=0.25,seed=3", "late=0.5,late=0.25", "early=3,efirst=0.02,elast=0.01", "seed=-1", "t60=0.3,t60=x", "t60= 1", "=3", "=x",
                "srctilt=5,srcaim=-30,src=hypercardioid,aim=200,tilt=10,mic=fig8/0.75,gain=0.2", "air=0/0.005/0.03,betas=0.9/0.8/0.6,xover=500/2000")],
    "plate": ["plate:", "plate:abc", "plate:0", "plate:-1",
              "plate:0.15:size=1.5,0.8,thick=1,material=70/2700/0.33,drive=0.5,0.3,pick=0.2,0.2/1.2,0.6,low=30,high=1200,t60=0.5/0.1,damp=1200,gain=0.02,last=0.1",
              "plate:0.1:gain=0.02,high=400",
              "plate:0.15:last=0.1,gain=0.02,damp=1200,t60=0.5/0.1,high=1200,low=30,pick=0.2,0.2/1.2,0.6,drive=0.5,0.3,material=70/2700/0.33,thick=1,size=1.5,0.8"]
             + ["plate:0.2" + t for t in ("", ":", ":size", ":size=2", ":size=2,1,3", ":size=2,x", ":thick=thin", ":thick=-1", ":material=brass", ":material=200/7850", ":drive=0.5",
                                          ":drive=0.5/0.4", ":pick=0.3,0.6", ":pick=0.3,0.6/1.5", ":pick=0.3/0.6/1.5/0.3", ":low=nan", ":high=-400", ":t60=4", ":t60=4,1",
                                          ":t60=4/-1", ":damp=inf", ":gain=1,5", ":last=-1", ":colour=3", ":late=0.1", ":gain=0.5,", ":,gain=0.5", ":gain=0.5:low=30",
                                          ":material=steel,t60=0/0", ":size=2,1,drive=0.5,0.25,gain=2", ":2,size=2,1", ":size=2,1,,gain=2", ":gain=2,size", ":colour=3,4")],
    "spring": ["spring:", "spring:abc", "spring:0", "spring:-1",
               "spring:0.15:sections=40,fc=3000,a=0.5,delay=21,27.5,33,t60=0.4,damping=0.1,lowpass=4,high=0.2,highsections=60,higha=-0.5,highdelay=0.4,hight60=0.2,"
               "stereo=0.05,gain=0.02,points=14,last=0.1", "spring:0.1:gain=0.02,delay=30",
               "spring:0.15:last=0.1,points=14,gain=0.02,stereo=0.05,hight60=0.2,highdelay=0.4,higha=-0.5,highsections=60,high=0.2,lowpass=4,damping=0.1,t60=0.4,"
               "delay=21,27.5,33,a=0.5,fc=3000,sections=40"]
              + ["spring:0.2" + t for t in ("", ":", ":delay", ":delay=", ":delay=66,x", ":delay=66,82,91,100", ":delay=66,0", ":delay=66/82", ":sections=many", ":sections=1.5",
                                            ":sections=-1", ":fc=nan", ":a=-0.5", ":t60=inf", ":damping=-0.1", ":lowpass=x", ":high=-1", ":highsections=2.5", ":higha=0.5",
                                            ":highdelay=", ":hight60=-1", ":stereo=wide", ":gain=1,5", ":points=-3", ":last=-1", ":colour=3", ":late=0.1", ":gain=0.5,",
                                            ":,gain=0.5", ":gain=0.5:fc=3000", ":delay=66,82,91,t60=0", ":high=0,lowpass=0,points=20", ":66,delay=30", ":delay=30,,gain=2",
                                            ":delay=30,40,delay=50")],
    "sweep": ["sweep:", "sweep:rec.wav", "sweep:rec.wav:0.1:100", "sweep::0.1:100:20000", "sweep:rec.wav:abc:100:20000", "sweep:rec.wav:0:100:20000",
              "sweep:rec.wav:-1:100:20000", "sweep:rec.wav:0.1:0.5:20000", "sweep:rec.wav:0.1:100:100", "sweep:rec.wav:0.1:100:20000x", "sweep:rec.wav:0.1:100:20000:",
              "sweep:rec.wav:0.1:100:20000:amp", "sweep:rec.wav:0.1:100:20000:amp=0", "sweep:rec.wav:0.1:100:20000:amp=-0.5", "sweep:rec.wav:0.1:100:20000:amp=0.5,",
              "sweep:rec.wav:0.1:100:20000:colour=3", "sweep:rec.wav:0.1:100:20000:fadein=-0.01", "sweep:rec.wav:0.1:100:20000:fadein=0.06,fadeout=0.05",
              "sweep:rec.wav:0.1:100:20000:offset=nan", "sweep:rec.wav:0.1:100:20000:length=-1", "sweep:rec.wav:0.1:100:20000:amp=0.5:offset=0",
              "sweep:rec.wav:0.085:100:20000:amp=0.25,fadein=0.001,fadeout=0.0005", "sweep:rec.wav:0.085:100:20000:amp=0.25,fadein=0.001,fadeout=0.0005,offset=-0.002,length=0.02",
              "sweep:rec.wav:0.5:100:3500:amp=0.25", "sweep:x.wav:0.05:20:20000", "sweep:x.wav:0.1:100", "sweep:x.wav:0:100:20000", "sweep:x.wav:0.1:100:30000",
              "sweep:x.wav:0.1:100:20000:amp=0", "sweep::0.1:100:20000",
              # fades longer than the sweep, either order, and exactly as long; F2 not above F1
              "sweep:rec.wav:0.1:100:20000:fadeout=0.05,fadein=0.06", "sweep:rec.wav:0.1:100:20000:fadein=0.05,fadeout=0.05", "sweep:rec.wav:0.1:100:20000:fadein=0.11",
              "sweep:rec.wav:0.1:100:20000:fadein=0.06,fadeout=0.05,colour=3", "sweep:rec.wav:0.1:100:99", "sweep:rec.wav:0.1:100:100.0001",
              "sweep:rec.wav:0.085:100:20000:length=0.02,offset=-0.002,fadeout=0.0005,fadein=0.001,amp=0.25"],
}


def _arg(grammar, items):
    return BASE[grammar] + (":" if BASE[grammar] else "") + items


def _with_ctx(k, item):
    return (k["ctx"] + "," if k["ctx"] else "") + item


def build_cases():
    """(cases, moves, by_key): every (grammar, group, argument), an argument once; per (grammar, key) the accepted argument and the
    same without the key's item; per (grammar, key) the arguments that vary that key's value."""
    cases, moves, by_key = [], {}, {}
    for g, keys in KEYS.items():
        for k in keys:
            name = k["key"]
            mine = by_key[(g, name)] = []
            values = [k["typical"]] + [v for edge in k["edges"] for v in edge] + list(k["more"]) + list(NUMS)
            for v in values:
                mine.append(_arg(g, _with_ctx(k, f"{name}={v}")))
            mine.append(_arg(g, _with_ctx(k, f"{name}={k['typical']},{name}={k['second']}")))
            # (a parts list cannot be empty: there the pair stands after an item that changes nothing)
            ctx = k["ctx"] or ("onset=0" if g == "parts" else "")
            moves[(g, name)] = (_arg(g, (ctx + "," if ctx else "") + f"{name}={k['typical']}"), _arg(g, ctx) if ctx else BASE[g])
            cases += [(g, "key " + name, a) for a in mine + list(moves[(g, name)])]
        # the structure of a list, with the first key's item as k=v
        kv = f"{keys[0]['key']}={keys[0]['typical']}"
        k, v = kv.split("=")
        for items in (k, "=" + v, kv + "=w", kv + ",", "," + kv, kv + ",," + kv, "colour=3", "colour=red", "colour=", "colour", kv + ",colour=3", "colour=3," + kv,
                      kv + ":" + kv, " " + kv, kv + " "):
            cases.append((g, "list", _arg(g, items)))
        cases += [(g, "list", ""), (g, "list", BASE[g]), (g, "list", BASE[g] + ":")]
    for g, (fields, swaps) in FIELDS.items():
        kv = f"{KEYS[g][0]['key']}={KEYS[g][0]['typical']}"
        for at, texts in swaps.items():
            for t in texts:
                line = ":".join(fields[:at] + [t] + fields[at + 1:])
                cases += [(g, "fields", line), (g, "fields", line + ":" + kv)]
        if len(fields) > 1:  # one field too few: the list stands where the last field should
            cases += [(g, "fields", ":".join(fields[:-1])), (g, "fields", ":".join(fields[:-1]) + ":" + kv)]
    for g, args in LITERAL.items():
        cases += [(g, "other", a) for a in args]
    for g, (typical, edges, more) in ONE.items():
        mine = by_key[(g, "")] = [typical] + [v for edge in edges for v in edge] + list(more) + list(NUMS)
        cases += [(g, "values", a) for a in mine]
    seen, unique = set(), []
    for g, group, a in cases:
        if (g, a) not in seen:
            seen.add((g, a))
            unique.append((g, group, a))
    return unique, moves, by_key


CASES, MOVES, BY_KEY = build_cases()
GRAMMARS = list(BASE) + list(ONE_VALUE)
LINE = re.compile(r'^(ok|refused) why="((?:[^"\\]|\\.)*)"((?: [A-Za-z0-9_.\[\]]+=(?:"(?:[^"\\]|\\.)*"|\S*))*)$')
MEMBER = re.compile(r' ([A-Za-z0-9_.\[\]]+)=("(?:[^"\\]|\\.)*"|\S*)')


def name_of(grammar, arg):
    """A case's name in the fixture: the argument, with ~ for the grammar's BASE at its front."""
    base = BASE.get(grammar)
    assert not arg.startswith("~")
    return "~" + arg[len(base):] if base and arg.startswith(base) else arg


def _split(line):
    m = LINE.match(line)
    assert m, line
    return m.group(1), m.group(2), m.group(3)


def compact(line, grammar):
    """The driver's line as the fixture stores it; `grammar` is the fixture's entry with form, refused and accepted."""
    status, why, members = _split(line)
    if status == "refused":
        assert members == grammar["refused"] and why, line  # (a refused argument leaves the default-constructed struct as it was)
        form = grammar["form"]
        return "refused " + (why.replace(form, "<form>") if form else why)
    assert not why, line
    members, base = MEMBER.findall(members), MEMBER.findall(grammar["accepted"] or "")
    assert not base or [n for n, _ in members] == [n for n, _ in base], line
    return "ok" + "".join(f" {n}={v}" for k, (n, v) in enumerate(members) if not base or v != base[k][1])


def expand(stored, grammar):
    """The whole line of a stored one."""
    if stored.startswith("refused "):
        return 'refused why="' + stored[8:].replace("<form>", grammar["form"]) + '"' + grammar["refused"]
    assert stored == "ok" or stored.startswith("ok "), stored
    if not grammar["accepted"]:
        return 'ok why=""' + stored[2:]
    given = dict(MEMBER.findall(stored[2:]))
    base = MEMBER.findall(grammar["accepted"])
    assert set(given) <= {n for n, _ in base}, stored
    return 'ok why=""' + "".join(f" {n}={given.get(n, d)}" for n, d in base)


def run_cases(binary):
    """{(grammar, argument): the driver's line} of every case."""
    def one(case):
        res = subprocess.run([binary, case[0], case[2]], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and res.stdout.endswith("\n") and res.stdout.count("\n") == 1 and not res.stderr, (case, res.returncode, res.stdout, res.stderr)
        return res.stdout[:-1]
    with ThreadPoolExecutor(8) as pool:
        return dict(zip(((g, a) for g, _, a in CASES), pool.map(one, CASES)))


@pytest.fixture(scope="module")
def fixture():
    """The fixture, and {(grammar, argument): stored line} of its cases."""
    with open(GOLDEN) as fh:
        f = json.load(fh)
    assert f["commit"] and list(f["grammars"]) == GRAMMARS
    stored = {}
    for g, entry in f["grammars"].items():
        assert (entry["accepted"] is None) == (g in WHOLE)
        for group, cases in entry["cases"].items():
            for name, line in cases.items():
                assert (g, group, name) not in stored
                stored[(g, group, name)] = line
    return f["grammars"], stored


@pytest.fixture(scope="module")
def got():
    subprocess.check_call(["make", "-C", HOST, "-s", "mcconv_parse_dump"])
    return run_cases(os.path.join(HOST, "mcconv_parse_dump"))


def test_the_cases_are_the_fixtures(fixture):
    names = [(g, group, name_of(g, a)) for g, group, a in CASES]
    assert len({(g, n) for g, _, n in names}) == len(names)
    assert set(names) == set(fixture[1])


@pytest.mark.parametrize("grammar", GRAMMARS)
def test_every_argument_parses_to_what_it_did(fixture, got, grammar):
    grammars, stored = fixture
    wrong = []
    for g, group, arg in CASES:
        if g != grammar:
            continue
        want = expand(stored[(g, group, name_of(g, arg))], grammars[g])
        if got[(g, arg)] != want:
            wrong.append((arg, got[(g, arg)], want))
    assert not wrong, (len(wrong), wrong[:5])


def _stored(fixture, grammar, arg):
    group = next(group for g, group, a in CASES if (g, a) == (grammar, arg))
    return fixture[1][(grammar, group, name_of(grammar, arg))]


def test_every_key_is_seen_to_move_a_field(fixture):
    """An accepted case whose dump differs from that of the same argument without the key's item."""
    assert set(MOVES) == {(g, k["key"]) for g, keys in KEYS.items() for k in keys}
    for (g, key), (with_item, without) in MOVES.items():
        a, b = (expand(_stored(fixture, g, arg), fixture[0][g]) for arg in (with_item, without))
        assert a.startswith("ok ") and b.startswith("ok ") and a != b, (g, key, a, b)
    for g, (typical, _, _) in ONE.items():
        a = expand(_stored(fixture, g, typical), fixture[0][g])
        assert a.startswith("ok ") and _split(a)[2] != fixture[0][g]["refused"], (g, a)


def test_every_key_has_a_refused_case(fixture):
    for (g, key), args in BY_KEY.items():
        assert any(_stored(fixture, g, a).startswith("refused ") for a in args), (g, key)


if __name__ == "__main__":
    lines = run_cases(os.path.abspath(sys.argv[3]))
    grammars = {}
    for g in GRAMMARS:
        dumps = {_split(l)[2] for (gg, a), l in lines.items() if gg == g and l.startswith("refused ")}
        assert len(dumps) == 1, (g, dumps)
        entry = grammars[g] = dict(form="", refused=dumps.pop(), accepted=None, cases={})
        if g in BASE:  # the form: what a refusal of an unknown key ends on
            why = _split(lines[(g, _arg(g, "colour=3"))])[1]
            index, option = "unknown key 'colour': ", "no such key 'colour' ("
            assert why.startswith(index) or (why.startswith(option) and why.endswith(")")), why
            entry["form"] = why[len(index):] if why.startswith(index) else why[len(option):-1]
        if g not in WHOLE:
            entry["accepted"] = _split(lines[(g, BASE[g])])[2] if BASE.get(g) else entry["refused"]
    for g, group, a in CASES:
        stored = grammars[g]["cases"].setdefault(group, {})[name_of(g, a)] = compact(lines[(g, a)], grammars[g])
        assert expand(stored, grammars[g]) == lines[(g, a)], (g, a)
    # one line per group of cases
    marks = {}
    for g, entry in grammars.items():
        for group, cases in entry["cases"].items():
            marks[f"@{len(marks)}@"] = cases
            entry["cases"][group] = f"@{len(marks) - 1}@"
    text = json.dumps(dict(commit=sys.argv[2], grammars=grammars), indent=1)
    for mark, cases in marks.items():
        text = text.replace(json.dumps(mark), json.dumps(cases))
    with open(sys.argv[1], "w") as fh:
        fh.write(text + "\n")
    print("recorded", len(CASES), "cases in", sys.argv[1], "from", sys.argv[3], "-", len(text), "bytes; whole lines would be", sum(len(l) + len(a) for (g, a), l in lines.items()))
