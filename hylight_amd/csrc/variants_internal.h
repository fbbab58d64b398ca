// variants_internal.h - what variants_host.cpp (the two entry points, the files) and variants.hip (the kernels) share.  The rules
// are those of include/hylight_mi.h (hlmi_variants, hlmi_variants_reads and their _ins forms); tests/variants_model.py and
// tests/variants_ins_model.py restate them.
#pragma once
#include <string_view>
#include <vector>

#include "common.h"
#include "polish_internal.h"
#include "variants_ins_text.h"
#include "variants_text.h"

namespace hlmi {
namespace var {

// The device part over the polisher's input (rows, compact CIGARs, reads as ASCII or codes, contig bytes, tiles, cbase - in.quals
// and in.min_cov are not read): the three counters per slot and the sites' records, ascending.  o: validated by the caller.
void variants_core(const pol::PolCoreIn &in, const hlmi_variant_opts &o, DeviceVariants &out);
// The same with the slots' counters in the one count pass (hlmi_variants_ins): `out` is what variants_core gives, except that
// tiles_revisited counts the tiles with a site of either kind; ins: slots_callable and ins_sites per slot, the insertion sites'
// records, ascending, finished on the device (variants_ins_text.h: InsRec).
void variants_ins_core(const pol::PolCoreIn &in, const hlmi_variant_opts &o, DeviceVariants &out, DeviceInsertions &ins);
// The two with the base-quality floor of the _q calls (variants_qual.h): min_base_qual in 1..93 and in.quals set - a column below
// the floor casts no vote (with the slots' counters it still spans), columns_low_qual gets the votes withheld, counted in the
// first pass alone.  min_base_qual == 0 or in.quals == nullptr: exactly the two above, columns_low_qual 0.
void variants_q_core(const pol::PolCoreIn &in, const hlmi_variant_opts &o, int min_base_qual, DeviceVariants &out,
                     uint64_t &columns_low_qual);
void variants_ins_q_core(const pol::PolCoreIn &in, const hlmi_variant_opts &o, int min_base_qual, DeviceVariants &out,
                         DeviceInsertions &ins, uint64_t &columns_low_qual);
// the option refusals of both entry points, in the header's order (hlmi_phase makes them first, under its own name)
void check_variant_opts(const char *who, const hlmi_variant_opts &o);
// the two refusals a _q call makes before anything is read: min_base_qual outside 0..93, min_avg_qual negative or not a number
void check_variant_qfloors(const char *who, const hlmi_variant_qopts &q);
// every contig record's length and bytes, as variants_text.h's and phase_text.h's functions take them
void contig_views(const SeqSet &cs, std::vector<uint64_t> &length, std::vector<std::string_view> &seq);

}  // namespace var

// pairs_paf, out_summary: may be nullptr
void variants_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                  const char *out_sites, const char *out_summary, hlmi_variant_stats *st);
void variants_reads_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                        const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st);
// the _ins forms: out_ins is not nullptr
void variants_ins_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_opts &o, const char *pairs_paf,
                      const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st);
void variants_reads_ins_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_opts &o,
                            const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                            hlmi_variant_ins_stats *st);
// the _q forms: the four above with the two floors of q, whose first five fields are o's; qc: the three counters
void variants_q_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts &q, const char *pairs_paf,
                    const char *out_sites, const char *out_summary, hlmi_variant_stats *st, hlmi_variant_qcounts *qc);
void variants_reads_q_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_qopts &q,
                          const char *pairs_paf, const char *out_sites, const char *out_summary, hlmi_variant_stats *st,
                          hlmi_variant_qcounts *qc);
void variants_ins_q_run(const char *contigs, const char *reads, const char *paf, const hlmi_variant_qopts &q, const char *pairs_paf,
                        const char *out_sites, const char *out_summary, const char *out_ins, hlmi_variant_ins_stats *st,
                        hlmi_variant_qcounts *qc);
void variants_reads_ins_q_run(const char *contigs, const char *reads, const hlmi_ava_opts &ao, const hlmi_variant_qopts &q,
                              const char *pairs_paf, const char *out_sites, const char *out_summary, const char *out_ins,
                              hlmi_variant_ins_stats *st, hlmi_variant_qcounts *qc);

}  // namespace hlmi
