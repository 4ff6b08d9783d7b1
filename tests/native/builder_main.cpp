// TEST INFRASTRUCTURE: the builder (fluidframework_amd/csrc/builder.cpp) as a stand-alone host program,
// built with AddressSanitizer and UBSan and linked without the HIP runtime and without libmte.so.
//
//   builder_main (doc OBSERVER LOG | summary OBSERVER SUMMARY LOG | open OBSERVER LOG1 LOG2)...
//
// doc: mte_builder_add_doc; summary: mte_builder_add_doc_from_summary; open: mte_builder_open_doc and
// the two files through mte_builder_append_messages (open documents come last). One
// mte_builder_batch at the end; prints "<array> <elements> <FNV-1a-64 of its bytes>" per batch array.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "../../include/mte.h"

static bool slurp(const char* path, std::string& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) {
        fprintf(stderr, "cannot read %s\n", path);
        return false;
    }
    out.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static void line(const char* name, const void* p, uint64_t count, size_t elem) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* b = (const unsigned char*)p;
    for (uint64_t i = 0; i < count * elem; i++) {
        h ^= b[i];
        h *= 0x100000001b3ull;
    }
    printf("%s %" PRIu64 " %016" PRIx64 "\n", name, count, h);
}

int main(int argc, char** argv) {
    mte_builder* b = nullptr;
    if (mte_builder_create(&b)) return 2;
    auto fail = [&](const char* what, int rc) {
        fprintf(stderr, "%s: %d: %s\n", what, rc, mte_builder_error(b));
        mte_builder_destroy(b);
        return 1;
    };
    for (int i = 1; i < argc;) {
        const std::string mode = argv[i];
        const int need = mode == "doc" ? 2 : (mode == "summary" || mode == "open") ? 3 : -1;
        if (need < 0 || i + need >= argc) {
            fprintf(stderr, "usage: builder_main (doc OBS LOG | summary OBS SUMMARY LOG | open OBS LOG1 LOG2)...\n");
            mte_builder_destroy(b);
            return 2;
        }
        const char* obs = argv[i + 1];
        std::string f1, f2;
        if (!slurp(argv[i + 2], f1) || (need == 3 && !slurp(argv[i + 3], f2))) {
            mte_builder_destroy(b);
            return 2;
        }
        int rc;
        if (mode == "doc") {
            if ((rc = mte_builder_add_doc(b, obs, f1.data(), f1.size()))) return fail("mte_builder_add_doc", rc);
        } else if (mode == "summary") {
            if ((rc = mte_builder_add_doc_from_summary(b, obs, f1.data(), f1.size(), f2.data(), f2.size())))
                return fail("mte_builder_add_doc_from_summary", rc);
        } else {
            uint32_t d = 0;
            if ((rc = mte_builder_open_doc(b, obs, &d))) return fail("mte_builder_open_doc", rc);
            if ((rc = mte_builder_append_messages(b, d, f1.data(), f1.size())) ||
                (rc = mte_builder_append_messages(b, d, f2.data(), f2.size())))
                return fail("mte_builder_append_messages", rc);
        }
        i += need + 1;
    }
    mte_batch v;
    memset(&v, 0, sizeof v);
    if (int rc = mte_builder_batch(b, &v)) return fail("mte_builder_batch", rc);
    const uint32_t n = v.n_docs;
    uint64_t nkv = 0;
    for (uint32_t i = 0; i < v.n_propsets; i++)
        if ((uint64_t)v.propsets[i].first + v.propsets[i].count > nkv) nkv = (uint64_t)v.propsets[i].first + v.propsets[i].count;
    const uint64_t names = v.doc_client_offsets[n];
    line("doc_op_offsets", v.doc_op_offsets, (uint64_t)n + 1, 8);
    line("ops", v.ops, v.doc_op_offsets[n], sizeof(mte_op));
    line("doc_payload_offsets", v.doc_payload_offsets, (uint64_t)n + 1, 8);
    line("payload", v.payload, v.doc_payload_offsets[n], 2);
    line("propsets", v.propsets, v.n_propsets, sizeof(mte_propset));
    line("prop_keys", v.prop_keys, nkv, 4);
    line("prop_vals", v.prop_vals, nkv, 4);
    line("key_offsets", v.key_offsets, (uint64_t)v.n_keys + 1, 8);
    line("key_text", v.key_text, v.key_offsets[v.n_keys], 1);
    line("val_offsets", v.val_offsets, (uint64_t)v.n_vals + 1, 8);
    line("val_text", v.val_text, v.val_offsets[v.n_vals], 1);
    line("doc_client_offsets", v.doc_client_offsets, (uint64_t)n + 1, 4);
    line("client_name_offsets", v.client_name_offsets, names + 1, 8);
    line("client_names", v.client_names, v.client_name_offsets[names], 1);
    mte_builder_destroy(b);
    return 0;
}
