// knobs.h -- fence around the developer knobs of the kernels (included first by engine.hip).
//
// kern_blindrot_pair.h carries `#ifdef ABLATION` switches that tools/ablate_k2.py sets with -D to time variants of the paired blind
// rotation: WRONG-RESULT modes (phases compiled out for a timing proxy).  EP_STAMPS adds per-phase cycle stamps to the three
// blind-rotation forms (tools/latency_stamps.py).  A product build must not be reachable by a stray -D: every knob named here is an
// #error unless the translation unit is compiled with -DFHEAES_DEV_BUILD, and fheaes_version() then says "dev"
// (tfhe_aes_amd/_native.py refuses such a library unless asked).  tests/test_cabi_cpu.py checks that this list names every knob the
// sources test and that _build.engine_flags() sets none.  (The equivalent-result tuning knobs of rounds 2-6 and the other ablations
// were retired once their experiments were closed: the measured best is the one code path, the numbers are in profiles/*_ablations.txt.)
#pragma once

#define FHEAES_KNOB_LIST(X) \
    X(EP_STAMPS) X(BRP_ABL_NOXSTORE) X(BRP_ABL_NODSTORE) X(BRP_ABL_NOBAR) X(BRP_ABL_NOPEEL) X(BRP_ABL_NOXREAD) X(BRP_ABL_SKEW) X(BRP_ABL_FEWCMUL) \
    X(BR16_ABL_NOLOAD) X(BR16_ABL_NOMAC) X(BR16_ABL_NOPARK)

#ifndef FHEAES_DEV_BUILD
#if defined(EP_STAMPS) || defined(BRP_ABL_NOXSTORE) || defined(BRP_ABL_NODSTORE) || defined(BRP_ABL_NOBAR) || defined(BRP_ABL_NOPEEL) || \
    defined(BRP_ABL_NOXREAD) || defined(BRP_ABL_SKEW) || defined(BRP_ABL_FEWCMUL) || defined(BR16_ABL_NOLOAD) || defined(BR16_ABL_NOMAC) || \
    defined(BR16_ABL_NOPARK)
#error "a developer knob of the kernels is defined on the command line: product builds take no knobs (add -DFHEAES_DEV_BUILD for a developer build; see csrc/knobs.h)"
#endif
#define FHEAES_BUILD_KIND ""
#else
#define FHEAES_BUILD_KIND " dev"
#endif
