// The k / v width a finalized plan carries, without a device (tests/test_gqa_host.py): encoder_model_check.cpp's protocol — "config H L HEADS FF VOCAB MAX_POS
// TYPE_VOCAB", then "setting NAME v...", "tensor NAME NUMEL", "finalize" — with one line per finalize only: "finalize rc=R kv_dim=A" (or "finalize rc=R msg").
// A load that is refused prints "refused NAME rc=R"; the bookkeeping is the loader's (encoder_weights.hpp) in its host-only part, as in that checker.
#include "../../kirag_amd/csrc/encoder_model.hpp"

#include <iostream>
#include <sstream>

using namespace kr::model;

int main() {
    kr_bert_cfg cfg{};
    std::string line, cmd, name;
    if (!std::getline(std::cin, line)) return 2;
    {
        std::istringstream in(line);
        if (!(in >> cmd >> cfg.hidden >> cfg.layers >> cfg.heads >> cfg.intermediate >> cfg.vocab >> cfg.max_pos >> cfg.type_vocab) || cmd != "config") return 2;
    }
    Settings set;
    Loaded ld(cfg.layers);
    bool finalized_once = false;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        if (!(in >> cmd)) continue;
        if (cmd == "finalize") {
            ModelPlan plan;
            const Error e = describe(cfg, set, ld, plan);
            if (e.code) std::cout << "finalize rc=" << e.code << " " << e.msg << "\n";
            else std::cout << "finalize rc=0 kv_dim=" << plan.kv_dim << "\n";
            finalized_once = finalized_once || e.code == 0;
            continue;
        }
        if (!(in >> name)) return 2;
        Error e;
        if (cmd == "setting") {
            std::vector<float> v;
            for (float x; in >> x;) v.push_back(x);
            bool stored = false;
            e = set_setting(cfg, set, ld.heads, finalized_once, name.c_str(), v.data(), (int64_t)v.size(), stored);
        } else if (cmd == "tensor") {
            long long numel = 0;
            if (!(in >> numel)) return 2;
            Resolved r;
            e = resolve_name(cfg, name.c_str(), r);
            if (!e.code) e = check_tensor(cfg, name.c_str(), r, numel, ld, finalized_once);
            if (!e.code) mark_loaded(ld, r);
        } else {
            return 2;
        }
        if (e.code) std::cout << "refused " << name << " rc=" << e.code << "\n";
    }
    return 0;
}
